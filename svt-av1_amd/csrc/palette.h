// palette.h — the arithmetic of the palette luma search that is the same on the host and on the device, written once (palette.hip runs it from one lane of a
// wave on LDS arrays, svt_hip_palette_search_host in svt_hip_host.cpp and tests/palette_host_test.cpp run it on the stack), and the whole search as a serial host
// form.  Plain C++17, no HIP.  File:line under Source/Lib of the reference:
//   Encoder/Codec/palette.c:18-24                 DIVIDE_AND_ROUND, lcg_rand16
//   Encoder/Codec/palette.c:72-153                av1_remove_duplicates, delta_encode_cost, svt_av1_index_color_cache, svt_av1_palette_color_cost_y
//   Encoder/Codec/palette.c:245-312               optimize_palette_colors, extend_palette_color_map, palette_rd_y
//   Encoder/Codec/palette.c:320-496               search_palette_luma
//   Encoder/Codec/k_means_template.h:23-133       svt_av1_calc_indices_dim1_c, calc_centroids, calc_total_dist, svt_av1_k_means_dim1_c
//   Encoder/Codec/EbPictureAnalysisProcess.c:3364-3399   svt_av1_count_colors[_highbd]
// No function here keeps an array of its own: whatever is indexed at run time is the caller's (LDS on the device, where a private array would live in scratch).
// docs/kernels/palette.md.
#pragma once
#include <stdint.h>
#include "../../include/svt_hip.h"
#if defined(__HIPCC__)
#define PAL_HD __host__ __device__ inline
#else
#define PAL_HD inline
#endif

namespace pal {

constexpr int MAX_SIZE = 8;                            // PALETTE_MAX_SIZE
constexpr int MAX_CANDS = SVT_HIP_PALETTE_MAX_CANDS;   // 7 dominant-colour slots, then 7 k-means slots
constexpr int MAX_COLORS = 64;                         // search_palette_luma: colors <= 64
constexpr int MAX_ITR = 50;                            // max_itr
constexpr int MAX_SAMPLES = 64 * 64;

PAL_HD uint32_t lcg_rand16(uint32_t* state) {
    *state = (uint32_t)(*state * 1103515245ULL + 12345);
    return *state / 65536 % 32768;
}
PAL_HD int div_round(int x, int y) { return (x + (y >> 1)) / y; }   // DIVIDE_AND_ROUND
PAL_HD int ceil_log2(int n) {                                      // av1_ceil_log2
    if (n < 2) return 0;
    int i = 1, p = 2;
    while (p < n) {
        i++;
        p = p << 1;
    }
    return i;
}

// the 16 shapes of svt_av1_allow_palette: the block sizes with both sides in 8 .. 64, and 4x16 / 16x4
PAL_HD bool shape_ok(int bw, int bh) {
    if ((bw == 4 && bh == 16) || (bw == 16 && bh == 4)) return true;
    if (bw < 8 || bh < 8 || bw > 64 || bh > 64 || (bw & (bw - 1)) || (bh & (bh - 1))) return false;
    return bw <= 4 * bh && bh <= 4 * bw;
}
PAL_HD bool job_ok(const SvtHipPaletteJob& j) {
    return shape_ok(j.bw, j.bh) && j.cols >= 1 && j.cols <= j.bw && j.rows >= 1 && j.rows <= j.bh && j.x >= 0 && j.y >= 0 && j.n_cache >= 0 && j.n_cache <= 16 &&
           (j.dominant_step == 1 || j.dominant_step == 2) && j.map_off >= 0;
}

// Candidate slot s: 0 .. 6 the dominant colours with n = nmax - s * step, 7 .. 13 k-means with n = nmax - (s - 7); the reference's order.  n < 2: the slot is empty.
PAL_HD int slot_kind(int s) { return s >= 7; }
PAL_HD int slot_n(int s, int nmax, int step) { return s >= 7 ? nmax - (s - 7) : nmax - s * step; }
// the initial centroid i of n between lb and ub
PAL_HD int init_centroid(int i, int n, int lb, int ub) { return lb + (2 * i + 1) * (ub - lb) / n / 2; }

// svt_av1_calc_indices_dim1_c for one sample: the first nearest of k centroids
PAL_HD int nearest(int v, const int* c, int k) {
    int best = 0, min_dist = (v - c[0]) * (v - c[0]);
    for (int j = 1; j < k; ++j) {
        const int d = (v - c[j]) * (v - c[j]);
        if (d < min_dist) {
            min_dist = d;
            best = j;
        }
    }
    return best;
}

// optimize_palette_colors: a centroid within 1 of a cache colour becomes that colour, the first nearest one
PAL_HD void snap_to_cache(const uint16_t* cache, int n_cache, int n, int* c) {
    if (n_cache <= 0) return;
    for (int i = 0; i < n; ++i) {
        int d0 = c[i] - (int)cache[0];
        int min_diff = d0 < 0 ? -d0 : d0, idx = 0;
        for (int j = 1; j < n_cache; ++j) {
            const int d = c[i] - (int)cache[j];
            const int this_diff = d < 0 ? -d : d;
            if (this_diff < min_diff) {
                min_diff = this_diff;
                idx = j;
            }
        }
        if (min_diff <= 1) c[i] = cache[idx];
    }
}

// av1_remove_duplicates: ascending order (the reference's qsort; equal integers have no order to keep), then the distinct values in front.  -> how many
PAL_HD int sort_dedup(int* c, int n) {
    for (int i = 1; i < n; ++i) {
        const int v = c[i];
        int j = i;
        for (; j > 0 && c[j - 1] > v; --j) c[j] = c[j - 1];
        c[j] = v;
    }
    int k = 1;
    for (int i = 1; i < n; ++i)
        if (c[i] != c[i - 1]) c[k++] = c[i];
    return k;
}

// delta_encode_cost; the deltas are taken from the colours again where the reference keeps them in an array
PAL_HD int delta_encode_cost(const int* colors, int num, int bit_depth, int min_val) {
    if (num <= 0) return 0;
    int bits_cost = bit_depth;
    if (num == 1) return bits_cost;
    bits_cost += 2;
    int max_delta = 0;
    const int min_bits = bit_depth - 3;
    for (int i = 1; i < num; ++i) {
        const int delta = colors[i] - colors[i - 1];
        if (delta > max_delta) max_delta = delta;
    }
    const int cl = ceil_log2(max_delta + 1 - min_val);
    int bits_per_delta = cl > min_bits ? cl : min_bits;
    int range = (1 << bit_depth) - colors[0] - min_val;
    for (int i = 0; i < num - 1; ++i) {
        bits_cost += bits_per_delta;
        range -= colors[i + 1] - colors[i];
        const int r = ceil_log2(range);
        bits_per_delta = bits_per_delta < r ? bits_per_delta : r;
    }
    return bits_cost;
}

// svt_av1_palette_color_cost_y: svt_av1_index_color_cache (the colours the cache does not hold go to `out`, 8 ints of the caller's), n_cache flag bits, the delta
// code of the rest, av1_cost_literal
PAL_HD int color_cost_y(const uint16_t* colors, int n, const uint16_t* cache, int n_cache, int bit_depth, int* out) {
    int n_out = 0;
    if (n_cache <= 0) {
        for (int i = 0; i < n; ++i) out[i] = colors[i];
        n_out = n;
    } else {
        int n_in_cache = 0;
        unsigned in_cache = 0;
        for (int i = 0; i < n_cache && n_in_cache < n; ++i)
            for (int j = 0; j < n; ++j)
                if (colors[j] == cache[i]) {
                    in_cache |= 1u << j;
                    ++n_in_cache;
                    break;
                }
        for (int i = 0; i < n; ++i)
            if (!((in_cache >> i) & 1)) out[n_out++] = colors[i];
    }
    const int total_bits = n_cache + delta_encode_cost(out, n_out, bit_depth, 1);
    return total_bits * (1 << 9);   // av1_cost_literal: AV1_PROB_COST_SHIFT
}

// The tail of a candidate, palette_rd_y up to the colour map: c[0 .. n) are the raw centroids on entry and the k sorted, distinct (unclipped: the map is taken
// from these) centroids on return; the record gets everything but its place in the output.  -> k, the palette size; the caller keeps the candidate when k > 2
// (k < 2 leaves palette_size 0 in the reference: not kept either way).  work: 8 ints.
PAL_HD int finish_candidate(int* c, int n, int kind, const uint16_t* cache, int n_cache, int bit_depth, int* work, SvtHipPaletteCand* rec) {
    for (int i = 0; i < MAX_SIZE; ++i) {
        rec->raw[i] = i < n ? (uint16_t)c[i] : 0;
        rec->colors[i] = 0;
    }
    rec->n = (uint8_t)n;
    rec->kind = (uint8_t)kind;
    rec->reserved = 0;
    rec->size = 0;
    rec->color_cost = 0;
    snap_to_cache(cache, n_cache, n, c);
    const int k = sort_dedup(c, n);
    if (k < 2) return k;
    const int max_val = (1 << bit_depth) - 1;
    for (int i = 0; i < k; ++i) rec->colors[i] = (uint16_t)(c[i] < 0 ? 0 : (c[i] > max_val ? max_val : c[i]));   // clip_pixel / clip_pixel_highbd
    rec->size = (uint8_t)k;
    rec->color_cost = color_cost_y(rec->colors, k, cache, n_cache, bit_depth, work);
    return k;
}

// One sample of the extended map (extend_palette_color_map): position p of the bw x bh block takes the sample of the last row / column inside rows x cols.
PAL_HD int extended_sample_index(int px, int py, int cols, int rows) { return (py < rows ? py : rows - 1) * cols + (px < cols ? px : cols - 1); }

#if !defined(__HIP_DEVICE_COMPILE__)
// ---------------------------------------------------------------------------------------------------------------- the serial host form
// svt_av1_k_means_dim1_c, sample by sample as the reference runs it (the device form takes the same sums over the block's histogram)
inline void k_means_host(const int* data, int* centroids, uint8_t* indices, uint8_t* pre_indices, int n, int k) {
    int pre_centroids[MAX_SIZE];
    const auto calc_indices = [&] { for (int i = 0; i < n; ++i) indices[i] = (uint8_t)nearest(data[i], centroids, k); };
    const auto total_dist = [&] {
        int64_t d = 0;
        for (int i = 0; i < n; ++i) d += (data[i] - centroids[indices[i]]) * (data[i] - centroids[indices[i]]);
        return d;
    };
    calc_indices();
    int64_t this_dist = total_dist();
    for (int it = 0; it < MAX_ITR; ++it) {
        const int64_t pre_dist = this_dist;
        for (int j = 0; j < k; ++j) pre_centroids[j] = centroids[j];
        for (int i = 0; i < n; ++i) pre_indices[i] = indices[i];
        int count[MAX_SIZE] = {0};
        uint32_t rand_state = (uint32_t)data[0];
        for (int j = 0; j < k; ++j) centroids[j] = 0;
        for (int i = 0; i < n; ++i) {
            ++count[indices[i]];
            centroids[indices[i]] += data[i];
        }
        for (int j = 0; j < k; ++j) centroids[j] = count[j] == 0 ? data[lcg_rand16(&rand_state) % n] : div_round(centroids[j], count[j]);
        calc_indices();
        this_dist = total_dist();
        if (this_dist > pre_dist) {
            for (int j = 0; j < k; ++j) centroids[j] = pre_centroids[j];
            for (int i = 0; i < n; ++i) indices[i] = pre_indices[i];
            break;
        }
        bool same = true;
        for (int j = 0; j < k; ++j) same = same && centroids[j] == pre_centroids[j];
        if (same) break;
    }
}

// search_palette_luma for one job
template <class PIX> inline void search_job_host(const PIX* plane, int stride, int bit_depth, const SvtHipPaletteJob& J, SvtHipPaletteResult* res, SvtHipPaletteCand* cands,
                                                 uint8_t* maps) {
    if (!job_ok(J)) {
        res->colors = -1;
        res->n_cands = 0;
        return;
    }
    static thread_local int     count_buf[1 << 10], data[MAX_SAMPLES];
    static thread_local uint8_t idx[MAX_SAMPLES], pre_idx[MAX_SAMPLES];
    const int  rows = J.rows, cols = J.cols, n_data = rows * cols, max_pix_val = 1 << bit_depth;
    const PIX* src = plane + (size_t)J.y * stride + J.x;
    res->n_cands = 0;
    for (int i = 0; i < max_pix_val; ++i) count_buf[i] = 0;
    int colors = 0;
    bool in_range = true;
    for (int r = 0; r < rows && in_range; ++r)
        for (int c = 0; c < cols; ++c) {
            const int v = src[(size_t)r * stride + c];
            if (v >= max_pix_val) {   // svt_av1_count_colors_highbd returns 0
                in_range = false;
                break;
            }
            ++count_buf[v];
        }
    if (in_range)
        for (int i = 0; i < max_pix_val; ++i) colors += count_buf[i] != 0;
    res->colors = colors;
    if (!(colors > 1 && colors <= MAX_COLORS)) return;
    int lb = src[0], ub = src[0];
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            const int v = src[(size_t)r * stride + c];
            data[r * cols + c] = v;
            if (v < lb) lb = v;
            else if (v > ub) ub = v;
        }
    const int nmax = colors < MAX_SIZE ? colors : MAX_SIZE;
    int top_colors[MAX_SIZE] = {0};
    for (int i = 0; i < nmax; ++i) {
        int max_count = 0;
        for (int j = 0; j < max_pix_val; ++j)
            if (count_buf[j] > max_count) {
                max_count = count_buf[j];
                top_colors[i] = j;
            }
        count_buf[top_colors[i]] = 0;
    }
    int tot = 0;
    for (int s = 0; s < MAX_CANDS; ++s) {
        const int n = slot_n(s, nmax, J.dominant_step), kind = slot_kind(s);
        if (n < 2) continue;
        int centroids[MAX_SIZE], work[MAX_SIZE];
        if (!kind) {
            for (int i = 0; i < n; ++i) centroids[i] = top_colors[i];
        } else if (colors == 2) {
            centroids[0] = lb;
            centroids[1] = ub;
        } else {
            for (int i = 0; i < n; ++i) centroids[i] = init_centroid(i, n, lb, ub);
            k_means_host(data, centroids, idx, pre_idx, n_data, n);
        }
        SvtHipPaletteCand* rec = cands + tot;
        const int k = finish_candidate(centroids, n, kind, J.cache, J.n_cache, bit_depth, work, rec);
        if (k <= 2) continue;
        uint8_t* map = maps + J.map_off + (size_t)tot * J.bw * J.bh;
        for (int py = 0; py < J.bh; ++py)
            for (int px = 0; px < J.bw; ++px) map[py * J.bw + px] = (uint8_t)nearest(data[extended_sample_index(px, py, cols, rows)], centroids, k);
        ++tot;
    }
    res->n_cands = tot;
}

inline bool search_args_ok(int pix_bytes, int bd, const void* plane, int stride, const void* jobs, int njobs, const void* results, const void* cands, const void* maps) {
    return plane && jobs && results && cands && maps && njobs >= 0 && stride > 0 && ((pix_bytes == 1 && bd == 8) || (pix_bytes == 2 && (bd == 8 || bd == 10)));
}
inline void search_host(int pix_bytes, int bd, const void* plane, int stride, const SvtHipPaletteJob* jobs, int njobs, SvtHipPaletteResult* results, SvtHipPaletteCand* cands,
                        uint8_t* maps) {
    for (int j = 0; j < njobs; ++j) {
        if (pix_bytes == 1) search_job_host((const uint8_t*)plane, stride, bd, jobs[j], results + j, cands + (size_t)j * MAX_CANDS, maps);
        else search_job_host((const uint16_t*)plane, stride, bd, jobs[j], results + j, cands + (size_t)j * MAX_CANDS, maps);
    }
}
#endif

}  // namespace pal
