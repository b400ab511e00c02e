// palette_host_test.cpp — svt-av1_amd/csrc/palette.h on host memory, built stand-alone (tests/test_palette_ref_cpu.py: plain and with
// -fsanitize=address,undefined).  An ordinary program: no Python, nothing preloaded.
//   <file> : six int32 (pix_bytes, bd, stride, plane rows, njobs, map bytes), the plane, the jobs, then the results, the 14 records per job and the maps that
//            svt_hip_palette_search_host left in zeroed buffers; the search is run again here into zeroed buffers and compared byte for byte
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../svt-av1_amd/csrc/palette.h"

static bool read_all(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[6];
    if (!read_all(f, hd, sizeof hd)) return 2;
    const int pix_bytes = hd[0], bd = hd[1], stride = hd[2], plane_rows = hd[3], njobs = hd[4], map_bytes = hd[5];
    const int slots = njobs > 0 ? njobs : 1;
    std::vector<uint8_t>             plane((size_t)stride * plane_rows * pix_bytes), want_maps(map_bytes), maps(map_bytes, 0);
    std::vector<SvtHipPaletteJob>    jobs(njobs);
    std::vector<SvtHipPaletteResult> want_res(slots), res(slots);
    std::vector<SvtHipPaletteCand>   want_cands((size_t)slots * pal::MAX_CANDS), cands((size_t)slots * pal::MAX_CANDS);
    if (!read_all(f, plane.data(), plane.size()) || !read_all(f, jobs.data(), jobs.size() * sizeof(SvtHipPaletteJob)) ||
        !read_all(f, want_res.data(), want_res.size() * sizeof(SvtHipPaletteResult)) || !read_all(f, want_cands.data(), want_cands.size() * sizeof(SvtHipPaletteCand)) ||
        !read_all(f, want_maps.data(), want_maps.size()))
        return 2;
    fclose(f);
    memset(res.data(), 0, res.size() * sizeof(SvtHipPaletteResult));
    memset(cands.data(), 0, cands.size() * sizeof(SvtHipPaletteCand));
    if (!pal::search_args_ok(pix_bytes, bd, plane.data(), stride, jobs.data(), njobs, res.data(), cands.data(), maps.data())) return 3;
    // exactly the bytes the jobs may touch: the sanitizer sees a store one byte outside the records or the maps
    pal::search_host(pix_bytes, bd, plane.data(), stride, jobs.data(), njobs, res.data(), cands.data(), maps.data());
    if (memcmp(res.data(), want_res.data(), res.size() * sizeof(SvtHipPaletteResult))) { printf("results differ\n"); return 1; }
    if (memcmp(cands.data(), want_cands.data(), cands.size() * sizeof(SvtHipPaletteCand))) { printf("records differ\n"); return 1; }
    if (maps != want_maps) { printf("maps differ\n"); return 1; }
    int kept = 0;
    for (int j = 0; j < njobs; ++j) kept += res[j].n_cands;
    printf("ok %d jobs, %d candidates kept\n", njobs, kept);
    return 0;
}
