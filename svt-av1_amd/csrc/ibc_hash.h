// ibc_hash.h — the arithmetic of the intra-block-copy hash table and hash search that is the same on the host and on the device, written once (ibc_hash.hip runs it
// per thread with the CRC tables in LDS, svt_hip_ibc_hash_table_host / svt_hip_ibc_hash_search_host in svt_hip_host.cpp and tests/ibc_hash_host_test.cpp run it
// serially with the tables in a constant), and both host forms.  Plain C++17, no HIP.  File:line under Source/Lib of the reference:
//   Encoder/Codec/hash.c:13-62                    the table-driven CRC: width 24, polynomials 0x5D6DCB / 0x864CFB, remainder reset per value
//   Encoder/Codec/hash_motion.c:138-251           svt_av1_generate_block_2x2_hash_value, svt_av1_generate_block_hash_value
//   Encoder/Codec/hash_motion.c:253-283           svt_av1_add_to_hash_map_by_row_with_precal_data
//   Encoder/Codec/hash_motion.c:285-369           svt_av1_get_block_hash_value
//   Encoder/Codec/av1me.c:273-282, :320-342, :1346-1403   mv_err_cost, is_mv_in, svt_av1_get_mvpred_var, the hash search of svt_av1_full_pixel_search
//   Encoder/Codec/EbAdaptiveMotionVectorPrediction.c:2003-2083   av1_is_dv_valid
//   Encoder/C_DEFAULT/EbComputeVariance_C.c:55-61   svt_aom_variance{N}x{N}_c
// The reference keeps the remainder in 32 bits and masks the result; only bits 16 .. 23 of a remainder choose the next table entry and bits above 23 never come
// back down, so the remainder is kept in 24 bits here.  docs/kernels/ibc_hash.md.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/svt_hip.h"
#if defined(__HIPCC__)
#define IBC_HD __host__ __device__ inline
#else
#define IBC_HD inline
#endif

namespace ibc {

constexpr uint32_t POLY1 = 0x5D6DCB, POLY2 = 0x864CFB, CRC_MASK = 0xFFFFFF;
constexpr int      KEY_CRC_BITS = 16;                      // crc_bits: the bucket key is (hash1 & 0xFFFF) + (size_index << 16)
constexpr int      N_BUCKETS = SVT_HIP_IBC_HASH_BUCKETS;   // 1 << (crc_bits + block_size_bits)
constexpr int      MAX_DIM = 32767;                        // BlockHash.x / .y are int16
constexpr int      MV_MAX = 16383;                         // a component table is addressed -MV_MAX .. MV_MAX
constexpr int      MAX_MIB_LOG2 = 16;

// crc_calculator_init_table, one entry
IBC_HD constexpr uint32_t crc_table_entry(uint32_t poly, uint32_t value) {
    uint32_t remainder = 0;
    for (uint32_t mask = 0x80; mask != 0; mask >>= 1) {
        if (value & mask) remainder ^= 1u << 23;
        remainder = (remainder & (1u << 23)) ? (remainder << 1) ^ poly : remainder << 1;
    }
    return remainder & CRC_MASK;
}
// crc_calculator_process_data over the four bytes of a little-endian word; T is anything indexed 0 .. 255
template <class T> IBC_HD uint32_t crc_word(const T& tab, uint32_t r, uint32_t w) {
    for (int i = 0; i < 4; ++i) {
        r = ((r << 8) & CRC_MASK) ^ tab[((r >> 16) ^ (w >> (8 * i))) & 0xFF];
    }
    return r;
}
// the CRC of a 2x2 block: its 4 sample bytes, or the 8 bytes of its four 16-bit samples in memory order
template <class PIX, class T> IBC_HD uint32_t crc_2x2(const T& tab, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3) {
    if (sizeof(PIX) == 1) return crc_word(tab, 0, p0 | (p1 << 8) | (p2 << 16) | (p3 << 24));
    return crc_word(tab, crc_word(tab, 0, p0 | (p1 << 16)), p2 | (p3 << 16));
}
// the CRC of the 16 bytes of four child hashes
template <class T> IBC_HD uint32_t crc_4(const T& tab, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    return crc_word(tab, crc_word(tab, crc_word(tab, crc_word(tab, 0, a), b), c), d);
}

IBC_HD int size_index(int block_size) {   // hash_block_size_to_index
    switch (block_size) {
    case 4: return 0;
    case 8: return 1;
    case 16: return 2;
    case 32: return 3;
    case 64: return 4;
    case 128: return 5;
    default: return -1;
    }
}
IBC_HD uint32_t bucket_key(uint32_t hash1, int size_idx) { return (hash1 & ((1u << KEY_CRC_BITS) - 1)) + ((uint32_t)size_idx << KEY_CRC_BITS); }
// same_info[2] of a block of `size` at (x, y): the position goes into the table
IBC_HD int add_flag(int same_row, int same_col, int x, int y, int size) { return (!same_row && !same_col) || (((x & (size - 1)) == 0) && ((y & (size - 1)) == 0)); }

IBC_HD bool fmt_ok(int pix_bytes, int bd) { return (pix_bytes == 1 && bd == 8) || (pix_bytes == 2 && (bd == 8 || bd == 10)); }
IBC_HD bool picture_ok(int stride, int width, int height) {
    return width >= 1 && height >= 1 && width <= MAX_DIM && height <= MAX_DIM && stride >= width && (int64_t)width * height <= INT32_MAX;
}
// the most entries a picture can have: every position of every size
inline int64_t max_entries(int width, int height) {
    int64_t n = 0;
    for (int s = 4; s <= 128; s *= 2)
        if (width >= s && height >= s) n += (int64_t)(width - s + 1) * (height - s + 1);
    return n;
}

// d_scratch of the table and of the block hashes, the same layout on both sides: two sets of planes (hash1, hash2 as words, three same_info planes as bytes), the
// records of the sort's first pass (packed position, hash2, the key's high byte), the per-workgroup digit counts of a sort pass, and the 65536 cursors of the host form's
// inserter.  Every part starts on a multiple of 256 bytes.
constexpr int SORT_TILE = 4096;   // positions per workgroup of a sort pass
struct ScratchLayout {
    size_t set[2], rec_xy, rec_h2, rec_hi, blockhist, cursor, total;
    int    nblocks;
};
inline ScratchLayout scratch_layout(int width, int height) {
    ScratchLayout L{};
    const size_t  n = (size_t)(width > 0 ? width : 0) * (size_t)(height > 0 ? height : 0);
    size_t        at = 0;
    const auto    take = [&](size_t bytes) { const size_t r = at; at += (bytes + 255) & ~(size_t)255; return r; };
    L.set[0] = take(11 * n);
    L.set[1] = take(11 * n);
    L.rec_xy = take(4 * n);
    L.rec_h2 = take(4 * n);
    L.rec_hi = take(n);
    L.nblocks = (int)((n + SORT_TILE - 1) / SORT_TILE);
    L.blockhist = take((size_t)L.nblocks * 256 * 4 + 4);
    L.cursor = take((size_t)(1 << KEY_CRC_BITS) * 4);
    L.total = at;
    return L;
}
inline void plane_set(uint8_t* scratch, const ScratchLayout& L, int i, int width, int height, uint32_t** h1, uint32_t** h2, int8_t* same[3]) {
    const size_t n = (size_t)width * height;
    uint8_t*     b = scratch + L.set[i];
    *h1 = (uint32_t*)b;
    *h2 = (uint32_t*)(b + 4 * n);
    for (int k = 0; k < 3; ++k) same[k] = (int8_t*)(b + (8 + k) * n);
}

// an entry the table's builder cannot have made is never followed: its block would lie outside the plane
IBC_HD bool entry_in_picture(int ex, int ey, int n, int width, int height) { return ex >= 0 && ey >= 0 && ex <= width - n && ey <= height - n; }

// ---------------------------------------------------------------------------------------------------------------- the search's arithmetic
IBC_HD bool tile_ok(int mi) { return mi >= 0 && mi <= (1 << 20); }   // keeps av1_is_dv_valid's edges inside 32 bits
IBC_HD bool job_ok(const SvtHipIbcSearchJob& j, int width, int height) {
    return size_index(j.block_size) >= 0 && j.x_pos >= 0 && j.y_pos >= 0 && j.x_pos <= width - j.block_size && j.y_pos <= height - j.block_size && j.mib_size_log2 >= 0 &&
           j.mib_size_log2 <= MAX_MIB_LOG2 && tile_ok(j.mi_row_start) && tile_ok(j.mi_row_end) && tile_ok(j.mi_col_start) && tile_ok(j.mi_col_end);
}
// av1_is_dv_valid for the block of job j and the entry at (ex, ey): 0 = valid, else the number of the rule that rejects (1 .. 4 the tile's top / left / bottom /
// right edge, 5 / 6 the sub-8x8 chroma rules, 7 the coded-superblock delay, 8 the wavefront, 9 the software wavefront).  dv is whole samples: the sub-pel rule
// cannot reject.
IBC_HD int dv_rule(const SvtHipIbcSearchJob& j, int ex, int ey) {
    const int bw = j.block_size, bh = j.block_size, mi_row = j.y_pos / 4, mi_col = j.x_pos / 4;
    const int dv_row = 8 * (ey - j.y_pos), dv_col = 8 * (ex - j.x_pos);
    const int src_top_edge = mi_row * 4 * 8 + dv_row, tile_top_edge = j.mi_row_start * 4 * 8;
    if (src_top_edge < tile_top_edge) return 1;
    const int src_left_edge = mi_col * 4 * 8 + dv_col, tile_left_edge = j.mi_col_start * 4 * 8;
    if (src_left_edge < tile_left_edge) return 2;
    const int src_bottom_edge = (mi_row * 4 + bh) * 8 + dv_row, tile_bottom_edge = j.mi_row_end * 4 * 8;
    if (src_bottom_edge > tile_bottom_edge) return 3;
    const int src_right_edge = (mi_col * 4 + bw) * 8 + dv_col, tile_right_edge = j.mi_col_end * 4 * 8;
    if (src_right_edge > tile_right_edge) return 4;
    // is_chroma_reference of a 4x4 block at 4:2:0: odd mi_row and odd mi_col
    if (bw < 8 && (mi_row & 1) && (mi_col & 1)) {
        if (src_left_edge < tile_left_edge + 4 * 8) return 5;
        if (src_top_edge < tile_top_edge + 4 * 8) return 6;
    }
    const int max_mib_size = 1 << j.mib_size_log2, active_sb_row = mi_row >> j.mib_size_log2, active_sb64_col = (mi_col * 4) >> 6, sb_size = max_mib_size * 4;
    const int src_sb_row = ((src_bottom_edge >> 3) - 1) / sb_size, src_sb64_col = ((src_right_edge >> 3) - 1) >> 6;
    const int total_sb64_per_row = ((j.mi_col_end - j.mi_col_start - 1) >> 4) + 1;
    const int active_sb64 = active_sb_row * total_sb64_per_row + active_sb64_col, src_sb64 = src_sb_row * total_sb64_per_row + src_sb64_col;
    if (src_sb64 >= active_sb64 - 4) return 7;   // INTRABC_DELAY_SB64
    const int gradient = 1 + 4 + (sb_size > 64), wf_offset = gradient * (active_sb_row - src_sb_row);
    if (src_sb_row > active_sb_row || src_sb64_col >= active_sb64_col - 4 + wf_offset) return 8;
    if (sb_size == 64) {
        if (src_sb64_col > active_sb64_col + (active_sb_row - src_sb_row)) return 9;
    } else {
        const int src_sb128_col = ((src_right_edge >> 3) - 1) >> 7, active_sb128_col = (mi_col * 4) >> 7;
        if (src_sb128_col > active_sb128_col + (active_sb_row - src_sb_row)) return 9;
    }
    return 0;
}
// is_mv_in: 0 = inside, else 1 .. 4 for col_min, col_max, row_min, row_max in the reference's order of tests
IBC_HD int mv_limit_rule(const SvtHipIbcSearchJob& j, int mv_row, int mv_col) {
    if (!(mv_col >= j.col_min)) return 1;
    if (!(mv_col <= j.col_max)) return 2;
    if (!(mv_row >= j.row_min)) return 3;
    if (!(mv_row <= j.row_max)) return 4;
    return 0;
}
// the two differences mv_err_cost looks up, in 1/8 sample; false when one is outside the tables (the reference would read outside them)
IBC_HD bool mv_diff(const SvtHipIbcSearchJob& j, int mv_row, int mv_col, int* d_row, int* d_col) {
    const int64_t r = (int64_t)mv_row * 8 - j.ref_mv_row, c = (int64_t)mv_col * 8 - j.ref_mv_col;
    if (r < -MV_MAX || r > MV_MAX || c < -MV_MAX || c > MV_MAX) return false;
    *d_row = (int)r;
    *d_col = (int)c;
    return true;
}
// mv_err_cost: svt_av1_get_mv_joint, mv_cost, ROUND_POWER_OF_TWO_64(cost * error_per_bit, RDDIV_BITS + AV1_PROB_COST_SHIFT - RD_EPB_SHIFT + 4)
IBC_HD int mv_err_cost(int d_row, int d_col, const int32_t* joint_cost, const int32_t* comp_cost, int error_per_bit) {
    const int     joint = d_row == 0 ? (d_col == 0 ? 0 : 1) : (d_col == 0 ? 2 : 3);
    const int32_t cost = joint_cost[joint] + comp_cost[MV_MAX + d_row] + comp_cost[SVT_HIP_IBC_MV_VALS + MV_MAX + d_col];
    return (int)(((int64_t)cost * error_per_bit + (1 << 13)) >> 14);
}
// the variance of an n x n block from its sum and sum of squares of differences: svt_aom_variance{n}x{n}_c at bit depth 8; at bit depth 10 the form of
// svt_aom_highbd_10_variance{n}x{n}_c (sse scaled by 1/16, the sum by 1/4, both rounded; not below 0)
IBC_HD uint32_t variance_of(int64_t sum, uint64_t sse, int n, int bd) {
    if (bd == 8) return (uint32_t)sse - (uint32_t)((sum * sum) / (n * n));
    const uint32_t sse10 = (uint32_t)((sse + 8) >> 4);
    const int64_t  sum10 = (sum + 2) >> 2;
    const int64_t  v = (int64_t)sse10 - (sum10 * sum10) / (n * n);
    return v >= 0 ? (uint32_t)v : 0;
}
// svt_av1_get_mvpred_var: unsigned variance + int cost, returned as int
IBC_HD int pred_cost(uint32_t var, int mv_cost) { return (int)(var + (uint32_t)mv_cost); }

IBC_HD SvtHipIbcSearchResult empty_result(int count) { return SvtHipIbcSearchResult{count, 0, 0, 0, INT32_MAX, 0, 0}; }

// ---------------------------------------------------------------------------------------------------------------- the serial host forms
struct CrcTable {
    uint32_t t[256];
    constexpr CrcTable(uint32_t poly) : t{} {
        for (uint32_t v = 0; v < 256; ++v) t[v] = crc_table_entry(poly, v);
    }
    constexpr uint32_t operator[](uint32_t i) const { return t[i]; }
};
inline const CrcTable& table1() { static constexpr CrcTable T(POLY1); return T; }
inline const CrcTable& table2() { static constexpr CrcTable T(POLY2); return T; }

// one picture-sized set of planes, indexed y * width + x
struct HostPlanes {
    uint32_t *h1, *h2;
    int8_t *  same[3];
};
template <class PIX> inline void level2_host(const PIX* luma, int stride, int width, int height, const HostPlanes& d) {
    for (int y = 0; y < height - 1; ++y)
        for (int x = 0; x < width - 1; ++x) {
            const PIX*     p = luma + (size_t)y * stride + x;
            const uint32_t p0 = p[0], p1 = p[1], p2 = p[stride], p3 = p[stride + 1];
            const size_t   pos = (size_t)y * width + x;
            d.same[0][pos] = p0 == p1 && p2 == p3;
            d.same[1][pos] = p0 == p2 && p1 == p3;
            d.h1[pos] = crc_2x2<PIX>(table1(), p0, p1, p2, p3);
            d.h2[pos] = crc_2x2<PIX>(table2(), p0, p1, p2, p3);
        }
}
inline void level_host(int width, int height, int size, const HostPlanes& s, const HostPlanes& d) {
    const int    half = size >> 1, quad = size >> 2;
    const size_t down = (size_t)half * width, qdown = (size_t)quad * width;
    for (int y = 0; y < height - size + 1; ++y)
        for (int x = 0; x < width - size + 1; ++x) {
            const size_t pos = (size_t)y * width + x;
            d.h1[pos] = crc_4(table1(), s.h1[pos], s.h1[pos + half], s.h1[pos + down], s.h1[pos + down + half]);
            d.h2[pos] = crc_4(table2(), s.h2[pos], s.h2[pos + half], s.h2[pos + down], s.h2[pos + down + half]);
            const int8_t *r = s.same[0], *c = s.same[1];
            d.same[0][pos] = r[pos] && r[pos + quad] && r[pos + half] && r[pos + down] && r[pos + down + quad] && r[pos + down + half];
            d.same[1][pos] = c[pos] && c[pos + half] && c[pos + qdown] && c[pos + qdown + half] && c[pos + down] && c[pos + down + half];
            d.same[2][pos] = (int8_t)add_flag(d.same[0][pos], d.same[1][pos], x, y, size);
        }
}

inline bool table_args_ok(int pix_bytes, int bd, const void* luma, int stride, int width, int height, const void* bucket_start, const void* entries, int64_t capacity,
                          const void* info, const void* scratch, size_t scratch_bytes) {
    return luma && bucket_start && info && scratch && (entries || capacity == 0) && capacity >= 0 && fmt_ok(pix_bytes, bd) && picture_ok(stride, width, height) &&
           scratch_bytes >= scratch_layout(width, height).total;
}
// the table of a picture: counts and starts always, the entries only when all of them fit.  Two runs over the levels: the first counts, the second stores each
// position behind its bucket's cursor in the inserter's order, column by column
inline void table_host(int pix_bytes, const void* luma, int stride, int width, int height, int32_t* bucket_start, SvtHipIbcHashEntry* entries, int64_t capacity,
                       int32_t* info, void* scratch) {
    const ScratchLayout L = scratch_layout(width, height);
    HostPlanes          pl[2];
    for (int i = 0; i < 2; ++i) plane_set((uint8_t*)scratch, L, i, width, height, &pl[i].h1, &pl[i].h2, pl[i].same);
    int32_t* cursor = (int32_t*)((uint8_t*)scratch + L.cursor);
    for (int k = 0; k <= N_BUCKETS; ++k) bucket_start[k] = 0;
    bool store = false;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) {
            int32_t run = 0;
            for (int k = 0; k < N_BUCKETS; ++k) {
                const int32_t c = bucket_start[k];
                bucket_start[k] = run;
                run += c;
            }
            bucket_start[N_BUCKETS] = run;
            store = run <= capacity;
            info[0] = run;
            info[1] = store;
            if (!store) return;
        }
        if (pix_bytes == 1) level2_host((const uint8_t*)luma, stride, width, height, pl[0]);
        else level2_host((const uint16_t*)luma, stride, width, height, pl[0]);
        int cur = 0;
        for (int size = 4; size <= 128 && size <= width && size <= height; size *= 2) {
            level_host(width, height, size, pl[cur], pl[cur ^ 1]);
            cur ^= 1;
            const int idx = size_index(size);
            if (store)
                for (int k = 0; k < (1 << KEY_CRC_BITS); ++k) cursor[k] = bucket_start[(idx << KEY_CRC_BITS) + k];
            for (int x = 0; x < width - size + 1; ++x)
                for (int y = 0; y < height - size + 1; ++y) {
                    const size_t pos = (size_t)y * width + x;
                    if (!pl[cur].same[2][pos]) continue;
                    const uint32_t key = bucket_key(pl[cur].h1[pos], idx);
                    if (store) entries[cursor[key & 0xFFFF]++] = SvtHipIbcHashEntry{(int16_t)x, (int16_t)y, pl[cur].h2[pos]};
                    else ++bucket_start[key];
                }
        }
    }
}

// svt_av1_get_block_hash_value of the n x n block at p: the two values of the pyramid's top.  buf: 2 * (n / 2)^2 + 2 * (n / 4)^2 words, the caller's
template <class PIX> inline void block_hash_host(const PIX* p, int stride, int n, uint32_t* buf, uint32_t* hash1, uint32_t* hash2) {
    int       w = n >> 1;
    uint32_t *a1 = buf, *a2 = a1 + w * w, *b1 = a2 + w * w, *b2 = b1 + (w >> 1) * (w >> 1);
    for (int y = 0; y < w; ++y)
        for (int x = 0; x < w; ++x) {
            const PIX*     q = p + (size_t)(2 * y) * stride + 2 * x;
            const uint32_t p0 = q[0], p1 = q[1], p2 = q[stride], p3 = q[stride + 1];
            a1[y * w + x] = crc_2x2<PIX>(table1(), p0, p1, p2, p3);
            a2[y * w + x] = crc_2x2<PIX>(table2(), p0, p1, p2, p3);
        }
    for (; w > 1; w >>= 1) {
        const int h = w >> 1;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < h; ++x) {
                const int s = 2 * y * w + 2 * x;
                b1[y * h + x] = crc_4(table1(), a1[s], a1[s + 1], a1[s + w], a1[s + w + 1]);
                b2[y * h + x] = crc_4(table2(), a2[s], a2[s + 1], a2[s + w], a2[s + w + 1]);
            }
        uint32_t* t = a1; a1 = b1; b1 = t;
        t = a2; a2 = b2; b2 = t;
    }
    *hash1 = a1[0];
    *hash2 = a2[0];
}

inline bool search_args_ok(int pix_bytes, int bd, const void* luma, int stride, int width, int height, const void* bucket_start, const void* entries,
                           const void* joint_cost, const void* comp_cost, const void* jobs, int njobs, const void* results) {
    return luma && bucket_start && entries && joint_cost && comp_cost && jobs && results && njobs >= 0 && fmt_ok(pix_bytes, bd) && picture_ok(stride, width, height);
}
template <class PIX> inline SvtHipIbcSearchResult search_job_host(const PIX* luma, int stride, int width, int height, int bd, const int32_t* bucket_start,
                                                                  const SvtHipIbcHashEntry* entries, const int32_t* joint_cost, const int32_t* comp_cost,
                                                                  const SvtHipIbcSearchJob& J, uint32_t* buf) {
    if (!job_ok(J, width, height)) return empty_result(-1);
    const int  n = J.block_size;
    const PIX* what = luma + (size_t)J.y_pos * stride + J.x_pos;
    uint32_t   h1, h2;
    block_hash_host(what, stride, n, buf, &h1, &h2);
    const uint32_t        key = bucket_key(h1, size_index(n));
    const int             first = bucket_start[key], count = bucket_start[key + 1] - first;
    SvtHipIbcSearchResult R = empty_result(count);
    if (count <= (J.intra ? 1 : 0)) return R;
    for (int i = 0; i < count; ++i) {
        const SvtHipIbcHashEntry e = entries[first + i];
        if (e.hash_value2 != h2) continue;
        ++R.n_matched;
        if (!entry_in_picture(e.x, e.y, n, width, height)) continue;
        if (J.intra && dv_rule(J, e.x, e.y)) continue;
        const int mv_row = e.y - J.y_pos, mv_col = e.x - J.x_pos;
        int       d_row, d_col;
        if (mv_limit_rule(J, mv_row, mv_col) || !mv_diff(J, mv_row, mv_col, &d_row, &d_col)) continue;
        ++R.n_valid;
        const PIX* cand = luma + (size_t)e.y * stride + e.x;
        int64_t    sum = 0;
        uint64_t   sse = 0;
        for (int y = 0; y < n; ++y)
            for (int x = 0; x < n; ++x) {
                const int d = (int)what[(size_t)y * stride + x] - (int)cand[(size_t)y * stride + x];
                sum += d;
                sse += (uint64_t)(d * d);
            }
        const int cost = pred_cost(variance_of(sum, sse, n, bd), mv_err_cost(d_row, d_col, joint_cost, comp_cost, J.error_per_bit));
        if (cost < R.best_cost) {
            R.found = 1;
            R.best_cost = cost;
            R.best_row = mv_row;
            R.best_col = mv_col;
        }
    }
    return R;
}
inline void search_host(int pix_bytes, int bd, const void* luma, int stride, int width, int height, const int32_t* bucket_start, const SvtHipIbcHashEntry* entries,
                        const int32_t* joint_cost, const int32_t* comp_cost, const SvtHipIbcSearchJob* jobs, int njobs, SvtHipIbcSearchResult* results) {
    static thread_local uint32_t buf[2 * 64 * 64 + 2 * 32 * 32];
    for (int j = 0; j < njobs; ++j)
        results[j] = pix_bytes == 1 ? search_job_host((const uint8_t*)luma, stride, width, height, bd, bucket_start, entries, joint_cost, comp_cost, jobs[j], buf)
                                    : search_job_host((const uint16_t*)luma, stride, width, height, bd, bucket_start, entries, joint_cost, comp_cost, jobs[j], buf);
}

}  // namespace ibc
