// ibc_search_host_test.cpp — svt-av1_amd/csrc/ibc_search.h on host memory, built stand-alone (tests/test_ibc_search_ref_cpu.py: plain and with
// -fsanitize=address,undefined).  An ordinary program: no Python, nothing preloaded.
//   <file> : eight int32 (pix_bytes, bd, stride, width, height, n_entries or -1 for "no table", njobs, 0), the eight int32 of the mesh patterns, the plane, the
//            cost tables (4 + 2 * 32767 int32), the jobs, the table when there is one (the bucket starts and exactly n_entries entries), then the njobs results
//            the library's host form left.  Every buffer here has exactly the size the contract names (the sanitizer sees a load or store one byte outside);
//            the search is run and compared byte for byte.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../svt-av1_amd/csrc/ibc_search.h"

static bool read_all(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[8], pat[8];
    if (!read_all(f, hd, sizeof hd) || !read_all(f, pat, sizeof pat)) return 2;
    const int  pix_bytes = hd[0], bd = hd[1], stride = hd[2], width = hd[3], height = hd[4], n_entries = hd[5], njobs = hd[6];
    const bool table = n_entries >= 0;
    std::vector<uint8_t>                   plane((size_t)stride * height * pix_bytes);
    std::vector<int32_t>                   joint(4), comp(2 * SVT_HIP_IBC_MV_VALS), start(table ? ibc::N_BUCKETS + 1 : 0);
    std::vector<SvtHipIbcFullSearchJob>    jobs(njobs);
    std::vector<SvtHipIbcHashEntry>        entries(table ? n_entries : 0);
    std::vector<SvtHipIbcFullSearchResult> want(njobs), res(njobs);
    if (!read_all(f, plane.data(), plane.size()) || !read_all(f, joint.data(), 16) || !read_all(f, comp.data(), comp.size() * 4) ||
        !read_all(f, jobs.data(), jobs.size() * sizeof(SvtHipIbcFullSearchJob)) || !read_all(f, start.data(), start.size() * 4) ||
        !read_all(f, entries.data(), entries.size() * sizeof(SvtHipIbcHashEntry)) || !read_all(f, want.data(), want.size() * sizeof(SvtHipIbcFullSearchResult)))
        return 2;
    fclose(f);
    static const SvtHipIbcHashEntry none{0, 0, 0};   // a table without entries still has a pointer: "both or neither"
    const int32_t*                  b = table ? start.data() : nullptr;
    const SvtHipIbcHashEntry*       e = table ? (entries.empty() ? &none : entries.data()) : nullptr;
    if (!ibcs::full_search_args_ok(pix_bytes, bd, plane.data(), stride, width, height, b, e, joint.data(), comp.data(), pat, jobs.data(), njobs, res.data())) return 3;
    if (ibcs::full_search_args_ok(pix_bytes, bd, plane.data(), stride, width, height, b, nullptr, joint.data(), comp.data(), pat, jobs.data(), njobs, res.data()) == table) return 3;
    memset(res.data(), 0xC3, res.size() * sizeof(SvtHipIbcFullSearchResult));
    ibcs::full_search_host(pix_bytes, bd, plane.data(), stride, width, height, b, e, joint.data(), comp.data(), pat, jobs.data(), njobs, res.data());
    for (int j = 0; j < njobs; ++j)
        if (memcmp(&res[j], &want[j], sizeof(SvtHipIbcFullSearchResult))) { printf("result %d differs\n", j); return 1; }
    int searched = 0, mesh = 0, hash = 0;
    for (int j = 0; j < njobs; ++j) {
        searched += res[j].status == 0;
        mesh += res[j].mesh_ran;
        hash += res[j].source == 2;
    }
    printf("ok %d jobs, %d searched, %d ran the mesh, %d took the hash result\n", njobs, searched, mesh, hash);
    return 0;
}
