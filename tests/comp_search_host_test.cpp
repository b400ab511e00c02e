// comp_search_host_test.cpp — svt-av1_amd/csrc/comp_search.h on host memory, built stand-alone (tests/test_comp_search_ref_cpu.py: plain and with
// -fsanitize=address,undefined).  An ordinary program: no Python, nothing preloaded.
//   <file> : eight int32 (pix_bytes, bd, stride, width, height, pred_samples, nrates, njobs), the three tables of the model (4 x 65 and 2 x 65 doubles, 22 int32),
//            the plane (stride x height samples), the predictor pool, the rates, the jobs, then what the library's host form left: the wedge mask table, the njobs
//            results and the 20 x njobs candidate records.  Every buffer here has exactly the size the contract names (the sanitizer sees a load or store one byte
//            outside); the table is built and the searches are run again and compared byte for byte.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../svt-av1_amd/csrc/comp_search.h"

static bool read_all(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[8];
    if (!read_all(f, hd, sizeof hd)) return 2;
    const int pix_bytes = hd[0], bd = hd[1], stride = hd[2], width = hd[3], height = hd[4], pred_samples = hd[5], nrates = hd[6], njobs = hd[7];
    std::vector<double>                 rate(cs::RATE_CATS * cs::GRID_COLS), dist(cs::DIST_CATS * cs::GRID_COLS);
    std::vector<int32_t>                cat(cs::BLOCK_SIZES), rates(nrates);
    std::vector<uint8_t>                plane((size_t)stride * height * pix_bytes), pool((size_t)pred_samples * pix_bytes), table(cs::WEDGE_TABLE_BYTES), mine(cs::WEDGE_TABLE_BYTES);
    std::vector<SvtHipCompSearchJob>    jobs(njobs);
    std::vector<SvtHipCompSearchResult> want(njobs), res(njobs);
    std::vector<SvtHipCompSearchCand>   want_c((size_t)njobs * cs::MAX_CANDS), cand((size_t)njobs * cs::MAX_CANDS);
    if (!read_all(f, rate.data(), rate.size() * 8) || !read_all(f, dist.data(), dist.size() * 8) || !read_all(f, cat.data(), cat.size() * 4) ||
        !read_all(f, plane.data(), plane.size()) || !read_all(f, pool.data(), pool.size()) || !read_all(f, rates.data(), rates.size() * 4) ||
        !read_all(f, jobs.data(), jobs.size() * sizeof(SvtHipCompSearchJob)) || !read_all(f, table.data(), table.size()) ||
        !read_all(f, want.data(), want.size() * sizeof(SvtHipCompSearchResult)) || !read_all(f, want_c.data(), want_c.size() * sizeof(SvtHipCompSearchCand)))
        return 2;
    fclose(f);
    cs::wedge_table_build(mine.data());
    if (memcmp(mine.data(), table.data(), table.size())) { printf("the wedge table differs\n"); return 1; }
    if (!cs::rd_tables_ok(rate.data(), dist.data(), cat.data()) ||
        !cs::search_args_ok(pix_bytes, bd, plane.data(), stride, width, height, pool.data(), pred_samples, rates.data(), nrates, jobs.data(), njobs, res.data()))
        return 3;
    // one sample less in the pool, one rate less: some job must now be refused (the lists end in the last predictor and use the last rate table)
    if (cs::search_args_ok(pix_bytes, bd, plane.data(), stride, width, height, pool.data(), pred_samples - 1, rates.data(), nrates, jobs.data(), njobs, res.data())) return 3;
    if (cs::search_args_ok(pix_bytes, bd, plane.data(), stride, width, height - 1, pool.data(), pred_samples, rates.data(), nrates, jobs.data(), njobs, res.data())) return 3;
    memset(res.data(), 0xC3, res.size() * sizeof(SvtHipCompSearchResult));
    memset(cand.data(), 0xC3, cand.size() * sizeof(SvtHipCompSearchCand));
    cs::search_host(pix_bytes, bd, plane.data(), stride, pool.data(), rates.data(), mine.data(), cs::RdTables{rate.data(), dist.data(), cat.data()}, jobs.data(), njobs, res.data(),
                    cand.data());
    for (int j = 0; j < njobs; ++j) {
        if (memcmp(&res[j], &want[j], sizeof(SvtHipCompSearchResult))) { printf("result %d differs\n", j); return 1; }
        if (memcmp(&cand[(size_t)j * cs::MAX_CANDS], &want_c[(size_t)j * cs::MAX_CANDS], cs::MAX_CANDS * sizeof(SvtHipCompSearchCand))) { printf("candidates of %d differ\n", j); return 1; }
    }
    int kinds[3] = {0, 0, 0};
    for (int j = 0; j < njobs; ++j) ++kinds[jobs[j].kind];
    printf("ok %d jobs: %d wedge, %d diff-weighted, %d inter-intra\n", njobs, kinds[0], kinds[1], kinds[2]);
    return 0;
}
