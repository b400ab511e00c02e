// ibc_hash_host_test.cpp — svt-av1_amd/csrc/ibc_hash.h on host memory, built stand-alone (tests/test_ibc_hash_ref_cpu.py: plain and with
// -fsanitize=address,undefined).  An ordinary program: no Python, nothing preloaded.
//   <file> : eight int32 (pix_bytes, bd, stride, width, height, n_entries, capacity, njobs), the plane, the cost tables (4 + 2 * 32767 int32), the jobs, then what
//            the library's host forms left: the bucket starts, the n_entries entries and the njobs results.  The table is built here twice, with exactly
//            `capacity` entries of room and with one fewer than it needs, into buffers of exactly the sizes the contract names (the sanitizer sees a store
//            one byte outside), the search is run on the table built here, and everything is compared byte for byte.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../svt-av1_amd/csrc/ibc_hash.h"

static bool read_all(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[8];
    if (!read_all(f, hd, sizeof hd)) return 2;
    const int pix_bytes = hd[0], bd = hd[1], stride = hd[2], width = hd[3], height = hd[4], n_entries = hd[5], capacity = hd[6], njobs = hd[7];
    std::vector<uint8_t>               plane((size_t)stride * height * pix_bytes);
    std::vector<int32_t>               joint(4), comp(2 * SVT_HIP_IBC_MV_VALS), want_start(ibc::N_BUCKETS + 1), start(ibc::N_BUCKETS + 1);
    std::vector<SvtHipIbcSearchJob>    jobs(njobs);
    std::vector<SvtHipIbcHashEntry>    want_entries(n_entries), entries(capacity);
    std::vector<SvtHipIbcSearchResult> want_res(njobs), res(njobs);
    if (!read_all(f, plane.data(), plane.size()) || !read_all(f, joint.data(), 16) || !read_all(f, comp.data(), comp.size() * 4) ||
        !read_all(f, jobs.data(), jobs.size() * sizeof(SvtHipIbcSearchJob)) || !read_all(f, want_start.data(), want_start.size() * 4) ||
        !read_all(f, want_entries.data(), want_entries.size() * sizeof(SvtHipIbcHashEntry)) || !read_all(f, want_res.data(), want_res.size() * sizeof(SvtHipIbcSearchResult)))
        return 2;
    fclose(f);
    const size_t         scratch_bytes = ibc::scratch_layout(width, height).total;
    std::vector<uint8_t> scratch(scratch_bytes);
    int32_t              info[2] = {-1, -1};
    if (!ibc::table_args_ok(pix_bytes, bd, plane.data(), stride, width, height, start.data(), entries.data(), capacity, info, scratch.data(), scratch_bytes)) return 3;
    if (ibc::table_args_ok(pix_bytes, bd, plane.data(), stride, width, height, start.data(), entries.data(), capacity, info, scratch.data(), scratch_bytes - 1)) return 3;
    if (n_entries > 0) {   // one entry short: the starts are complete, nothing is stored
        std::vector<SvtHipIbcHashEntry> few(n_entries - 1);
        ibc::table_host(pix_bytes, plane.data(), stride, width, height, start.data(), few.data(), n_entries - 1, info, scratch.data());
        if (info[0] != n_entries || info[1] != 0 || start != want_start) { printf("short table differs\n"); return 1; }
    }
    ibc::table_host(pix_bytes, plane.data(), stride, width, height, start.data(), entries.data(), capacity, info, scratch.data());
    if (info[0] != n_entries || info[1] != (n_entries <= capacity)) { printf("info differs: %d %d\n", info[0], info[1]); return 1; }
    if (start != want_start) { printf("bucket starts differ\n"); return 1; }
    if (n_entries > 0 && n_entries <= capacity && memcmp(entries.data(), want_entries.data(), want_entries.size() * sizeof(SvtHipIbcHashEntry))) { printf("entries differ\n"); return 1; }
    if (n_entries <= capacity && njobs > 0) {
        if (!ibc::search_args_ok(pix_bytes, bd, plane.data(), stride, width, height, start.data(), entries.data(), joint.data(), comp.data(), jobs.data(), njobs, res.data())) return 3;
        ibc::search_host(pix_bytes, bd, plane.data(), stride, width, height, start.data(), entries.data(), joint.data(), comp.data(), jobs.data(), njobs, res.data());
        if (memcmp(res.data(), want_res.data(), res.size() * sizeof(SvtHipIbcSearchResult))) { printf("results differ\n"); return 1; }
    }
    int found = 0;
    for (int j = 0; j < njobs; ++j) found += res[j].found;
    printf("ok %d entries, %d jobs, %d found\n", n_entries, njobs, found);
    return 0;
}
