// ifs_search_host_test.cpp — svt-av1_amd/csrc/ifs_search.h on host memory, built stand-alone (tests/test_ifs_ref_cpu.py: plain and with
// -fsanitize=address,undefined).  An ordinary program: no Python, nothing preloaded.
//   <file> : eight int32 (pix_bytes, bd, width, height, src_stride, njobs, two reference pictures 0 / 1, model points), the source plane (src_stride x height samples),
//            reference picture 0 and, if present, 1 WITH their border: (height + 7) x (width + 7) samples each, the picture at (3, 3), which is exactly the contracted 3
//            samples left and above and 4 right and below (the sanitizer sees a load one sample outside); the jobs; then what the library's host form left: the njobs
//            results, the 9 x njobs candidate records and the width x height destination plane (started as zeros); then the model points, three int64 (var, n_log2,
//            qstep) each, and their expected two int64 (rate, dist).  The searches and the model are run again and compared byte for byte.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../svt-av1_amd/csrc/ifs_search.h"

static bool read_all(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[8];
    if (!read_all(f, hd, sizeof hd)) return 2;
    const int pix_bytes = hd[0], bd = hd[1], width = hd[2], height = hd[3], src_stride = hd[4], njobs = hd[5], two = hd[6], npoints = hd[7];
    const int rstride = width + ifs::REACH_LO + ifs::REACH_HI, rrows = height + ifs::REACH_LO + ifs::REACH_HI;
    std::vector<uint8_t>         src((size_t)src_stride * height * pix_bytes), ref0((size_t)rstride * rrows * pix_bytes), ref1(two ? ref0.size() : 0);
    std::vector<uint8_t>         want_dst((size_t)width * height * pix_bytes), dst(want_dst.size(), 0);
    std::vector<SvtHipIfsJob>    jobs(njobs);
    std::vector<SvtHipIfsResult> want(njobs), res(njobs);
    std::vector<SvtHipIfsCand>   want_c((size_t)njobs * ifs::NCAND), cand(want_c.size());
    std::vector<int64_t>         points((size_t)npoints * 3), want_p((size_t)npoints * 2);
    if (!read_all(f, src.data(), src.size()) || !read_all(f, ref0.data(), ref0.size()) || !read_all(f, ref1.data(), ref1.size()) ||
        !read_all(f, jobs.data(), jobs.size() * sizeof(SvtHipIfsJob)) || !read_all(f, want.data(), want.size() * sizeof(SvtHipIfsResult)) ||
        !read_all(f, want_c.data(), want_c.size() * sizeof(SvtHipIfsCand)) || !read_all(f, want_dst.data(), want_dst.size()) || !read_all(f, points.data(), points.size() * 8) ||
        !read_all(f, want_p.data(), want_p.size() * 8))
        return 2;
    fclose(f);
    const size_t origin = ((size_t)ifs::REACH_LO * rstride + ifs::REACH_LO) * pix_bytes;
    const void * r0 = ref0.data() + origin, *r1 = two ? ref1.data() + origin : nullptr;
    if (!ifs::search_args_ok(pix_bytes, bd, src.data(), src_stride, width, height, r0, rstride, r1, rstride, dst.data(), width, jobs.data(), njobs, res.data())) return 3;
    // a row less of source: some job must now be refused (the lists have blocks in the bottom corners)
    if (ifs::search_args_ok(pix_bytes, bd, src.data(), src_stride, width, height - 1, r0, rstride, r1, rstride, dst.data(), width, jobs.data(), njobs, res.data())) return 3;
    memset(res.data(), 0xC3, res.size() * sizeof(SvtHipIfsResult));
    memset(cand.data(), 0xC3, cand.size() * sizeof(SvtHipIfsCand));
    ifs::search_host(pix_bytes, bd, src.data(), src_stride, r0, rstride, r1, rstride, dst.data(), width, jobs.data(), njobs, res.data(), cand.data());
    for (int j = 0; j < njobs; ++j) {
        if (memcmp(&res[j], &want[j], sizeof(SvtHipIfsResult))) { printf("result %d differs\n", j); return 1; }
        if (memcmp(&cand[(size_t)j * ifs::NCAND], &want_c[(size_t)j * ifs::NCAND], ifs::NCAND * sizeof(SvtHipIfsCand))) { printf("candidates of %d differ\n", j); return 1; }
    }
    if (memcmp(dst.data(), want_dst.data(), dst.size())) { printf("the destination plane differs\n"); return 1; }
    for (int p = 0; p < npoints; ++p) {
        int32_t rate;
        int64_t dist;
        ifs::model_rd_from_var_lapndz(points[3 * p], (uint32_t)points[3 * p + 1], (uint32_t)points[3 * p + 2], &rate, &dist);
        if (rate != want_p[2 * p] || dist != want_p[2 * p + 1]) { printf("model point %d differs\n", p); return 1; }
    }
    int refs[2] = {0, 0};
    for (int j = 0; j < njobs; ++j) ++refs[jobs[j].type >= 0];
    printf("ok %d jobs: %d of one reference, %d of two; %d model points\n", njobs, refs[0], refs[1], npoints);
    return 0;
}
