// ibc_hash.hip — the intra-block-copy hash planes and hash table of a picture and the hash search of a list of blocks on gfx950 (wave64), behind
// svt_hip_ibc_block_hashes_dev, svt_hip_ibc_hash_table_dev and svt_hip_ibc_hash_search_batch_dev.
//
// Replaces (file:line under Source/Lib of the reference):
//   Encoder/Codec/hash_motion.c:138-251           svt_av1_generate_block_2x2_hash_value, svt_av1_generate_block_hash_value
//   Encoder/Codec/hash_motion.c:253-283           svt_av1_add_to_hash_map_by_row_with_precal_data (six calls, EbModeDecisionConfigurationProcess.c:939-1051)
//   Encoder/Codec/av1me.c:1346-1403               the hash search of svt_av1_full_pixel_search, with svt_av1_get_block_hash_value (hash_motion.c:285-369),
//                                                 av1_is_dv_valid, is_mv_in, svt_av1_get_mvpred_var
//
// Planes: a thread per position and level, the two 256-entry CRC tables in LDS (each thread makes one entry of each on the way in), the arithmetic from ibc_hash.h.
// A level reads its four children and writes 11 bytes per position; the levels are separate launches over global planes (no LDS tile with a halo yet:
// docs/kernels/ibc_hash.md).
//
// Table: the levels run twice.  The first run only counts: every position that is to be added bumps its bucket's counter in d_bucket_start (integer adds: the
// counts do not depend on their order), one workgroup scans the counters to the starts and writes {n_entries, stored}.  The second run makes each level's planes
// again and sorts the level's added positions by their 16 key bits with a stable two-pass radix sort (8 bits a pass) over the positions enumerated column by column,
// which is the inserter's order: per pass a workgroup counts the digits of its tile, one workgroup scans the digit-major counts, and one wave per tile places its
// elements chunk by chunk, 64 at a time, ranking equal digits inside a chunk by ballots.  No atomic decides a place.  A level's buckets are contiguous and in key
// order, so the second pass writes entry r of the level at d_bucket_start[size_index << 16] + r.  Nothing of the second run stores when stored = 0.
//
// Search: a workgroup of four waves per job.  The block's 2x2 CRCs go to LDS and are folded there level by level.  Each wave takes 64 entries of the bucket at a
// time, a lane an entry (hash_value2, av1_is_dv_valid, is_mv_in); the survivors are costed one after the other by the whole wave (a lane a sample, sums by
// shuffles).  A wave meets its entries in ascending order and keeps the first smallest cost; the four waves' results meet by (cost, bucket index).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svt_hip_internal.h"
#include "fmt_dispatch.h"
#include "lane_reduce.h"
#include "ibc_hash.h"

namespace {

#define PD __device__ __forceinline__

constexpr int WG = 256, WAVES = WG / 64;

struct Planes {
    uint32_t *h1, *h2;
    int8_t *  s0, *s1, *s2;
};

PD void wave_sync() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }

// both CRC tables into LDS by a workgroup of 256 threads; the caller synchronises
PD void make_tables(uint32_t* t1, uint32_t* t2, int tid) {
    t1[tid] = ibc::crc_table_entry(ibc::POLY1, (uint32_t)tid);
    t2[tid] = ibc::crc_table_entry(ibc::POLY2, (uint32_t)tid);
}

// ---------------------------------------------------------------------------------------------------------------- the hash planes
template <class PIX> __global__ __launch_bounds__(WG) void ibc_level2_kernel(const PIX* __restrict__ luma, int stride, int width, int x_end, int y_end, Planes d) {
    __shared__ uint32_t t1[256], t2[256];
    make_tables(t1, t2, threadIdx.y * 64 + threadIdx.x);
    __syncthreads();
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= x_end || y >= y_end) return;
    const PIX*     p = luma + (size_t)y * stride + x;
    const uint32_t p0 = p[0], p1 = p[1], p2 = p[stride], p3 = p[stride + 1];
    const size_t   pos = (size_t)y * width + x;
    d.s0[pos] = p0 == p1 && p2 == p3;
    d.s1[pos] = p0 == p2 && p1 == p3;
    d.h1[pos] = ibc::crc_2x2<PIX>(t1, p0, p1, p2, p3);
    d.h2[pos] = ibc::crc_2x2<PIX>(t2, p0, p1, p2, p3);
}

// one level: the block of `size` at every position from the four blocks of size / 2.  counts: the table's bucket counters, or null
__global__ __launch_bounds__(WG) void ibc_level_kernel(int width, int x_end, int y_end, int size, Planes s, Planes d, int32_t* __restrict__ counts) {
    __shared__ uint32_t t1[256], t2[256];
    make_tables(t1, t2, threadIdx.y * 64 + threadIdx.x);
    __syncthreads();
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= x_end || y >= y_end) return;
    const int      half = size >> 1, quad = size >> 2;
    const size_t   pos = (size_t)y * width + x, down = (size_t)half * width, qdown = (size_t)quad * width;
    const uint32_t h1 = ibc::crc_4(t1, s.h1[pos], s.h1[pos + half], s.h1[pos + down], s.h1[pos + down + half]);
    const uint32_t h2 = ibc::crc_4(t2, s.h2[pos], s.h2[pos + half], s.h2[pos + down], s.h2[pos + down + half]);
    const int8_t * r = s.s0, *c = s.s1;
    const int      same_row = r[pos] && r[pos + quad] && r[pos + half] && r[pos + down] && r[pos + down + quad] && r[pos + down + half];
    const int      same_col = c[pos] && c[pos + half] && c[pos + qdown] && c[pos + qdown + half] && c[pos + down] && c[pos + down + half];
    const int      add = ibc::add_flag(same_row, same_col, x, y, size);
    d.h1[pos] = h1;
    d.h2[pos] = h2;
    d.s0[pos] = (int8_t)same_row;
    d.s1[pos] = (int8_t)same_col;
    d.s2[pos] = (int8_t)add;
    if (counts && add) atomicAdd(&counts[ibc::bucket_key(h1, ibc::size_index(size))], 1);
}

// ---------------------------------------------------------------------------------------------------------------- scan
// exclusive prefix sums of a[0 .. n) in place, one workgroup: a thread sums a contiguous part, the 1024 sums are scanned in LDS, the thread writes its part.
// info, if given, receives {the total, total <= capacity}.
constexpr int SCAN_WG = 1024;
__global__ __launch_bounds__(SCAN_WG) void ibc_scan_kernel(int32_t* __restrict__ a, int n, int32_t* __restrict__ info, long long capacity) {
    __shared__ int32_t s[SCAN_WG];
    const int t = threadIdx.x, per = (n + SCAN_WG - 1) / SCAN_WG;
    const int lo = min(n, t * per), hi = min(n, lo + per);
    int32_t   sum = 0;
    for (int i = lo; i < hi; ++i) sum += a[i];
    s[t] = sum;
    __syncthreads();
    for (int step = 1; step < SCAN_WG; step <<= 1) {
        const int32_t v = t >= step ? s[t - step] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    int32_t run = s[t] - sum;
    for (int i = lo; i < hi; ++i) {
        const int32_t v = a[i];
        a[i] = run;
        run += v;
    }
    if (info && t == 0) {
        const int32_t total = s[SCAN_WG - 1];
        info[0] = total;
        info[1] = (long long)total <= capacity;
    }
}

// ---------------------------------------------------------------------------------------------------------------- the stable sort of a level
struct SortArgs {
    Planes                p;                          // the level's planes
    int                   width, y_end, n_level;      // positions of the level, enumerated i = x * y_end + y
    int                   size_idx, nblocks;          // nblocks: tiles of ibc::SORT_TILE positions, the same for both passes
    uint32_t *            rec_xy, *rec_h2;            // pass 0 -> pass 1: the added positions ordered by the key's low byte
    uint8_t*              rec_hi;
    int32_t*              blockhist;                  // [256][nblocks] digit counts, scanned in place
    const int32_t*        bucket_start;               // scanned
    const int32_t*        info;                       // {n_entries, stored}
    SvtHipIbcHashEntry*   entries;
};
struct SortElem {
    uint32_t digit, xy, h2, hi;
};
// element i of pass PASS; false when there is none (pass 0: the position is not added)
template <int PASS> PD bool sort_load(const SortArgs& a, int i, int n, SortElem* e) {
    if (i >= n) return false;
    if (PASS == 0) {
        const int    x = i / a.y_end, y = i - x * a.y_end;
        const size_t pos = (size_t)y * a.width + x;
        if (!a.p.s2[pos]) return false;
        const uint32_t h1 = a.p.h1[pos];
        *e = SortElem{h1 & 0xFF, ((uint32_t)x << 15) | (uint32_t)y, a.p.h2[pos], (h1 >> 8) & 0xFF};
    } else {
        const uint32_t hi = a.rec_hi[i];
        *e = SortElem{hi, a.rec_xy[i], a.rec_h2[i], hi};
    }
    return true;
}
template <int PASS> PD int sort_count(const SortArgs& a) {
    return PASS == 0 ? a.n_level : a.bucket_start[(a.size_idx + 1) << ibc::KEY_CRC_BITS] - a.bucket_start[a.size_idx << ibc::KEY_CRC_BITS];
}

template <int PASS> __global__ __launch_bounds__(WG) void ibc_sort_hist_kernel(SortArgs a) {
    __shared__ int32_t hist[256];
    const int tid = threadIdx.x, b = blockIdx.x;
    hist[tid] = 0;
    __syncthreads();
    if (a.info[1]) {   // the same for every thread
        const int n = sort_count<PASS>(a), first = b * ibc::SORT_TILE;
        for (int i = first + tid; i < first + ibc::SORT_TILE; i += WG) {
            SortElem e;
            if (sort_load<PASS>(a, i, n, &e)) atomicAdd(&hist[e.digit], 1);
        }
    }
    __syncthreads();
    a.blockhist[(size_t)tid * a.nblocks + b] = hist[tid];
}

// one wave per tile: off[d] is where the tile's next element of digit d goes
template <int PASS> __global__ __launch_bounds__(64) void ibc_sort_scatter_kernel(SortArgs a) {
    __shared__ int32_t off[256];
    const int lane = threadIdx.x, b = blockIdx.x;
    if (!a.info[1]) return;
    for (int d = lane; d < 256; d += 64) off[d] = a.blockhist[(size_t)d * a.nblocks + b];
    wave_sync();
    const int n = sort_count<PASS>(a), first = b * ibc::SORT_TILE;
    const int level_base = a.bucket_start[a.size_idx << ibc::KEY_CRC_BITS];
    if (first >= n) return;
    for (int base = first; base < first + ibc::SORT_TILE && base < n; base += 64) {
        SortElem   e{0, 0, 0, 0};
        const bool have = sort_load<PASS>(a, base + lane, n, &e);
        // the lanes of this chunk with the same digit
        unsigned long long same = __ballot(have);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool               set = (e.digit >> bit) & 1;
            const unsigned long long m = __ballot(set);
            same &= set ? m : ~m;
        }
        const int rank = __popcll(same & ((1ull << lane) - 1));
        const int at = have ? off[e.digit] + rank : 0;
        wave_sync();
        if (have && rank == 0) off[e.digit] += __popcll(same);   // one lane per digit present
        wave_sync();
        if (have) {
            if (PASS == 0) {
                a.rec_xy[at] = e.xy;
                a.rec_h2[at] = e.h2;
                a.rec_hi[at] = (uint8_t)e.hi;
            } else {
                a.entries[(size_t)level_base + at] = SvtHipIbcHashEntry{(int16_t)(e.xy >> 15), (int16_t)(e.xy & 0x7FFF), e.h2};
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the search
struct WaveBest {
    int cost, index, row, col, n_matched, n_valid;
};

template <class PIX, int BD> __global__ __launch_bounds__(WG) void ibc_search_kernel(const PIX* __restrict__ luma, int stride, int width, int height,
                                                                                     const int32_t* __restrict__ bucket_start, const SvtHipIbcHashEntry* __restrict__ entries,
                                                                                     const int32_t* __restrict__ joint_cost, const int32_t* __restrict__ comp_cost,
                                                                                     const SvtHipIbcSearchJob* __restrict__ jobs, SvtHipIbcSearchResult* __restrict__ results) {
    __shared__ uint32_t           t1[256], t2[256];
    __shared__ uint32_t           s_a[2][64 * 64], s_b[2][32 * 32];   // the block's hash pyramid: levels alternate between the two
    __shared__ SvtHipIbcSearchJob s_job;
    __shared__ WaveBest           s_best[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, job = blockIdx.x;
    static_assert(sizeof(SvtHipIbcSearchJob) % 4 == 0 && sizeof(SvtHipIbcSearchJob) / 4 <= WG, "copied by words");
    if (tid < (int)(sizeof(SvtHipIbcSearchJob) / 4)) ((uint32_t*)&s_job)[tid] = ((const uint32_t*)(jobs + job))[tid];
    make_tables(t1, t2, tid);
    __syncthreads();
    const SvtHipIbcSearchJob J = s_job;
    if (!ibc::job_ok(J, width, height)) {   // the same for every thread
        if (tid == 0) results[job] = ibc::empty_result(-1);
        return;
    }
    const int  n = J.block_size, n_log2 = __ffs(n) - 1;
    const PIX* what = luma + (size_t)J.y_pos * stride + J.x_pos;
    int        w = n >> 1, w_log2 = n_log2 - 1;
    for (int i = tid; i < w * w; i += WG) {
        const int      y = i >> w_log2, x = i & (w - 1);
        const PIX*     q = what + (size_t)(2 * y) * stride + 2 * x;
        const uint32_t p0 = q[0], p1 = q[1], p2 = q[stride], p3 = q[stride + 1];
        s_a[0][i] = ibc::crc_2x2<PIX>(t1, p0, p1, p2, p3);
        s_a[1][i] = ibc::crc_2x2<PIX>(t2, p0, p1, p2, p3);
    }
    __syncthreads();
    int in_a = 1;   // the current level is in s_a
    for (; w > 1; w >>= 1, --w_log2) {
        const int       h = w >> 1, h_log2 = w_log2 - 1;
        const uint32_t *c1 = in_a ? s_a[0] : s_b[0], *c2 = in_a ? s_a[1] : s_b[1];
        uint32_t *      d1 = in_a ? s_b[0] : s_a[0], *d2 = in_a ? s_b[1] : s_a[1];
        for (int i = tid; i < h * h; i += WG) {
            const int y = i >> h_log2, x = i & (h - 1), s = 2 * y * w + 2 * x;
            d1[i] = ibc::crc_4(t1, c1[s], c1[s + 1], c1[s + w], c1[s + w + 1]);
            d2[i] = ibc::crc_4(t2, c2[s], c2[s + 1], c2[s + w], c2[s + w + 1]);
        }
        __syncthreads();
        in_a ^= 1;
    }
    const uint32_t hash1 = in_a ? s_a[0][0] : s_b[0][0], hash2 = in_a ? s_a[1][0] : s_b[1][0];
    const uint32_t key = ibc::bucket_key(hash1, ibc::size_index(n));
    const int      first = bucket_start[key], count = bucket_start[key + 1] - first;
    if (count <= (J.intra ? 1 : 0)) {
        if (tid == 0) results[job] = ibc::empty_result(count);
        return;
    }
    WaveBest best{INT32_MAX, INT32_MAX, 0, 0, 0, 0};
    for (int base = wave * 64; base < count; base += WG) {
        const int          i = base + lane;
        SvtHipIbcHashEntry e{0, 0, 0};
        if (i < count) e = entries[(size_t)first + i];
        const bool matched = i < count && e.hash_value2 == hash2;
        const int  mv_row = e.y - J.y_pos, mv_col = e.x - J.x_pos;
        int        d_row = 0, d_col = 0;
        const bool ok = matched && ibc::entry_in_picture(e.x, e.y, n, width, height) && !(J.intra && ibc::dv_rule(J, e.x, e.y)) && !ibc::mv_limit_rule(J, mv_row, mv_col) &&
                        ibc::mv_diff(J, mv_row, mv_col, &d_row, &d_col);
        best.n_matched += __popcll(__ballot(matched));
        unsigned long long todo = __ballot(ok);
        best.n_valid += __popcll(todo);
        while (todo) {   // the same for every lane
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int  ex = __shfl((int)e.x, src, 64), ey = __shfl((int)e.y, src, 64), c_row = __shfl(d_row, src, 64), c_col = __shfl(d_col, src, 64);
            const PIX* cand = luma + (size_t)ey * stride + ex;
            int        sum = 0;        // at most 256 samples a lane: |sum| <= 256 * 1023, sse <= 256 * 1023^2 < 2^32
            uint32_t   sse = 0;
            for (int k = lane; k < n * n; k += 64) {
                const int    y = k >> n_log2, x = k & (n - 1);
                const size_t o = (size_t)y * stride + x;
                const int    d = (int)what[o] - (int)cand[o];
                sum += d;
                sse += (uint32_t)(d * d);
            }
            const long long          tot_sum = wave_sum_i64((long long)sum);
            const unsigned long long tot_sse = wave_sum_u64((unsigned long long)sse);
            const int cost = ibc::pred_cost(ibc::variance_of(tot_sum, tot_sse, n, BD), ibc::mv_err_cost(c_row, c_col, joint_cost, comp_cost, J.error_per_bit));
            if (cost < best.cost) best = WaveBest{cost, base + src, ey - J.y_pos, ex - J.x_pos, best.n_matched, best.n_valid};
        }
    }
    if (lane == 0) s_best[wave] = best;
    __syncthreads();
    if (tid == 0) {
        SvtHipIbcSearchResult R = ibc::empty_result(count);
        int                   index = INT32_MAX;
        for (int v = 0; v < WAVES; ++v) {
            const WaveBest b = s_best[v];
            R.n_matched += b.n_matched;
            R.n_valid += b.n_valid;
            if (b.index != INT32_MAX && (b.cost < R.best_cost || (b.cost == R.best_cost && b.index < index))) {
                R.best_cost = b.cost;
                R.best_row = b.row;
                R.best_col = b.col;
                index = b.index;
            }
        }
        R.found = R.n_valid > 0;
        results[job] = R;
    }
}

Planes scratch_planes(void* scratch, const ibc::ScratchLayout& L, int i, int width, int height) {
    Planes  p;
    int8_t* same[3];
    ibc::plane_set((uint8_t*)scratch, L, i, width, height, &p.h1, &p.h2, same);
    p.s0 = same[0];
    p.s1 = same[1];
    p.s2 = same[2];
    return p;
}
dim3 plane_grid(int x_end, int y_end) { return dim3((x_end + 63) / 64, (y_end + 3) / 4); }

void launch_level2(hipStream_t st, int pix_bytes, const void* luma, int stride, int width, int height, const Planes& d) {
    svt_for_pix(pix_bytes, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        hipLaunchKernelGGL((ibc_level2_kernel<PIX>), plane_grid(width - 1, height - 1), dim3(64, 4), 0, st, (const PIX*)luma, stride, width, width - 1, height - 1, d);
    });
}
void launch_level(hipStream_t st, int width, int height, int size, const Planes& s, const Planes& d, int32_t* counts) {
    hipLaunchKernelGGL(ibc_level_kernel, plane_grid(width - size + 1, height - size + 1), dim3(64, 4), 0, st, width, width - size + 1, height - size + 1, size, s, d, counts);
}

}  // namespace

int svt_hip_launch_ibc_block_hashes(hipStream_t st, int pix_bytes, const void* luma, int stride, int width, int height, int block_size, uint32_t* hash1, uint32_t* hash2,
                                    int8_t* same, void* scratch) {
    if (width < block_size || height < block_size) return (int)hipSuccess;
    const ibc::ScratchLayout L = ibc::scratch_layout(width, height);
    const size_t             n = (size_t)width * height;
    const Planes             out{hash1, hash2, same, same + n, same + 2 * n};
    const Planes             set[2] = {scratch_planes(scratch, L, 0, width, height), scratch_planes(scratch, L, 1, width, height)};
    launch_level2(st, pix_bytes, luma, stride, width, height, block_size == 2 ? out : set[0]);
    int cur = 0;
    for (int size = 4; size <= block_size; size *= 2) {
        launch_level(st, width, height, size, set[cur], size == block_size ? out : set[cur ^ 1], nullptr);
        cur ^= 1;
    }
    return (int)hipGetLastError();
}

int svt_hip_launch_ibc_hash_table(hipStream_t st, int pix_bytes, const void* luma, int stride, int width, int height, int32_t* bucket_start, SvtHipIbcHashEntry* entries,
                                  int64_t capacity, int32_t* info, void* scratch) {
    const ibc::ScratchLayout L = ibc::scratch_layout(width, height);
    const Planes             set[2] = {scratch_planes(scratch, L, 0, width, height), scratch_planes(scratch, L, 1, width, height)};
    const hipError_t         e = hipMemsetAsync(bucket_start, 0, (size_t)(ibc::N_BUCKETS + 1) * sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    const bool any = width >= 4 && height >= 4;
    for (int run = 0; run < 2 && any; ++run) {
        if (run == 1) hipLaunchKernelGGL(ibc_scan_kernel, dim3(1), dim3(SCAN_WG), 0, st, bucket_start, ibc::N_BUCKETS + 1, info, (long long)capacity);
        launch_level2(st, pix_bytes, luma, stride, width, height, set[0]);
        int cur = 0;
        for (int size = 4; size <= 128 && size <= width && size <= height; size *= 2) {
            launch_level(st, width, height, size, set[cur], set[cur ^ 1], run == 0 ? bucket_start : nullptr);
            cur ^= 1;
            if (run == 0) continue;
            SortArgs a;
            a.p = set[cur];
            a.width = width;
            a.y_end = height - size + 1;
            a.n_level = (width - size + 1) * a.y_end;
            a.size_idx = ibc::size_index(size);
            a.nblocks = (a.n_level + ibc::SORT_TILE - 1) / ibc::SORT_TILE;   // <= L.nblocks
            a.rec_xy = (uint32_t*)((uint8_t*)scratch + L.rec_xy);
            a.rec_h2 = (uint32_t*)((uint8_t*)scratch + L.rec_h2);
            a.rec_hi = (uint8_t*)scratch + L.rec_hi;
            a.blockhist = (int32_t*)((uint8_t*)scratch + L.blockhist);
            a.bucket_start = bucket_start;
            a.info = info;
            a.entries = entries;
            hipLaunchKernelGGL(ibc_sort_hist_kernel<0>, dim3(a.nblocks), dim3(WG), 0, st, a);
            hipLaunchKernelGGL(ibc_scan_kernel, dim3(1), dim3(SCAN_WG), 0, st, a.blockhist, 256 * a.nblocks, (int32_t*)nullptr, 0ll);
            hipLaunchKernelGGL(ibc_sort_scatter_kernel<0>, dim3(a.nblocks), dim3(64), 0, st, a);
            hipLaunchKernelGGL(ibc_sort_hist_kernel<1>, dim3(a.nblocks), dim3(WG), 0, st, a);
            hipLaunchKernelGGL(ibc_scan_kernel, dim3(1), dim3(SCAN_WG), 0, st, a.blockhist, 256 * a.nblocks, (int32_t*)nullptr, 0ll);
            hipLaunchKernelGGL(ibc_sort_scatter_kernel<1>, dim3(a.nblocks), dim3(64), 0, st, a);
        }
    }
    if (!any) hipLaunchKernelGGL(ibc_scan_kernel, dim3(1), dim3(SCAN_WG), 0, st, bucket_start, ibc::N_BUCKETS + 1, info, (long long)capacity);
    return (int)hipGetLastError();
}

int svt_hip_launch_ibc_hash_search(hipStream_t st, int pix_bytes, int bd, const void* luma, int stride, int width, int height, const int32_t* bucket_start,
                                   const SvtHipIbcHashEntry* entries, const int32_t* joint_cost, const int32_t* comp_cost, const SvtHipIbcSearchJob* jobs, int njobs,
                                   SvtHipIbcSearchResult* results) {
    svt_for_fmt(pix_bytes, bd, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        hipLaunchKernelGGL((ibc_search_kernel<PIX, (decltype(f)::bd)>), dim3(njobs), dim3(WG), 0, st, (const PIX*)luma, stride, width, height, bucket_start, entries, joint_cost,
                           comp_cost, jobs, results);
    });
    return (int)hipGetLastError();
}

SVT_HIP_TU_PROBE(ibc_hash)
