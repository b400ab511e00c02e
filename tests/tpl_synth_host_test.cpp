// tpl_synth_host_test.cpp — svt-av1_amd/csrc/tpl_synth.h on host memory, built stand-alone (tests/test_tpl_synth_host.py: plain and with
// -fsanitize=address,undefined).  Every buffer is a heap block of exactly the size the ABI names, so a read or write past a grid, a record array or the output
// is an AddressSanitizer report.
//   no argument : the closed forms of tests/tpl_synth_common.py (chain, single scatters, truncation) against the numbers stored below
//   <file>      : a window dumped by tests/test_tpl_synth_host.py with the expected grids and output; compared byte for byte
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../svt-av1_amd/csrc/tpl_synth.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

struct Window {
    SvtHipTplSynthParams p{};
    std::vector<SvtHipTplMbStats*> stats;
    std::vector<int64_t*> dep;
    std::vector<SvtHipTplWindowFrame> frames;
    void* out = nullptr;
    size_t n_mb = 0, dep_bytes = 0, out_bytes = 0;

    Window(int w, int h, int cell_log2, int sb_size, int rm, double r0_in, int n) {
        p.w = w; p.h = h; p.cell_log2 = cell_log2; p.sb_size = sb_size; p.base_rdmult = rm; p.rate = 0; p.r0_in = r0_in;
        n_mb = (size_t)((w + 15) / 16) * ((h + 15) / 16);
        dep_bytes = tplsyn::dep_cells(tplsyn::geom(w, h, cell_log2)) * 2 * sizeof(int64_t);
        out_bytes = tplsyn::out_bytes(w, h, sb_size);
        out = std::malloc(out_bytes);
        for (int i = 0; i < n; i++) {
            stats.push_back((SvtHipTplMbStats*)std::calloc(n_mb, sizeof(SvtHipTplMbStats)));
            dep.push_back((int64_t*)std::malloc(dep_bytes));
            std::memset(dep.back(), 0x5A, dep_bytes);   // the call zeroes the grids
            SvtHipTplWindowFrame f{};
            f.d_stats = stats.back(); f.d_dep = dep.back(); f.on = 1;
            for (int k = 0; k < 8; k++) f.ref_window[k] = -1;
            frames.push_back(f);
        }
    }
    ~Window() {
        for (auto s : stats) std::free(s);
        for (auto d : dep) std::free(d);
        std::free(out);
    }
    void fill(int i, int64_t sd, int64_t rd, int64_t sr, int64_t rr, int rf_idx) {
        for (size_t k = 0; k < n_mb; k++) {
            SvtHipTplMbStats& s = stats[i][k];
            s.srcrf_dist = sd; s.recrf_dist = rd; s.srcrf_rate = sr; s.recrf_rate = rr; s.rf_idx = (int8_t)rf_idx;
        }
    }
    bool run() {
        if (!tplsyn::params_ok(&p) || tplsyn::frames_check(frames.data(), (int)frames.size())) return false;
        tplsyn::window_host(p, frames.data(), (int)frames.size(), out);
        return true;
    }
    const SvtHipTplR0BetaHeader& head() const { return *(const SvtHipTplR0BetaHeader*)out; }
    const double* factors() const { return (const double*)((const char*)out + sizeof(SvtHipTplR0BetaHeader)); }
    const double* beta() const { return factors() + n_mb; }
};

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// tests/tpl_synth_common.py: chain_case and CHAIN_*
void chain() {
    Window W(40, 24, 3, 64, 100, 0.75, 4);
    for (int i = 0; i < 4; i++) {
        W.fill(i, 1000, 2000, 7, 7, 0);
        W.frames[i].ref_window[1] = i - 1;   // picture 0's slot names a POC outside the window
    }
    CHECK(W.run());
    const int64_t dep[4] = {1750, 1500, 1000, 0};
    for (int i = 0; i < 4; i++)
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 6; c++) {
                CHECK(W.dep[i][2 * (r * 6 + c)] == 0);
                CHECK(W.dep[i][2 * (r * 6 + c) + 1] == (r < 3 && c < 5 ? dep[i] : 0));
            }
    CHECK(W.head().intra_cost_base == 18 * 256000 && W.head().mc_dep_cost_base == 18 * 256000 + 15 * 224000);
    const double r0 = 4608000.0 / 7968000.0;
    CHECK(same_bits(W.head().r0, r0));
    const double f[6] = {(1024000.0 / 1920000.0) / r0 + 1.2, (1024000.0 / 1920000.0) / r0 + 1.2, (1024000.0 / 1472000.0) / r0 + 1.2,
                         (512000.0 / 960000.0) / r0 + 1.2,   (512000.0 / 960000.0) / r0 + 1.2,   (512000.0 / 736000.0) / r0 + 1.2};
    for (int k = 0; k < 6; k++) CHECK(same_bits(W.factors()[k], f[k]));
    CHECK(same_bits(W.beta()[0], r0 / (6144000.0 / 9504000.0)));
}

struct Add { int row, col; int64_t rate, dist; };
// tests/tpl_synth_common.py: single_case and SINGLE
void single(int mb_row, int mb_col, int mv_row, int mv_col, int64_t sd, int64_t rd, int64_t sr, int64_t rr, const std::vector<Add>& adds) {
    Window W(64, 64, 4, 64, 1234, 0.75, 2);
    W.fill(0, 1, 1, 1, 1, 0);
    W.fill(1, 1, 1, 1, 1, 0);
    W.frames[1].ref_window[1] = 0;
    SvtHipTplMbStats& s = W.stats[1][mb_row * 4 + mb_col];
    s.srcrf_dist = sd; s.recrf_dist = rd; s.srcrf_rate = sr; s.recrf_rate = rr; s.mv_row = (int16_t)mv_row; s.mv_col = (int16_t)mv_col; s.is_inter = 1;
    CHECK(W.run());
    int64_t want[2][16][2] = {};
    for (const Add& a : adds) { want[0][a.row * 4 + a.col][0] = a.rate; want[0][a.row * 4 + a.col][1] = a.dist; }
    for (int i = 0; i < 2; i++) CHECK(std::memcmp(W.dep[i], want[i], sizeof want[i]) == 0);
}

void closed_forms() {
    chain();
    single(1, 1, 128, -128, 100, 612, 10, 266, {{2, 0, 256, 512}});
    single(1, 1, 43, -21, 100, 612, 10, 266, {{1, 0, 33, 66}, {1, 1, 143, 286}, {2, 0, 15, 30}, {2, 1, 65, 130}});
    single(0, 0, -40, -24, 100, 612, 10, 266, {{0, 0, 143, 286}});
    single(3, 3, 40, 24, 100, 612, 10, 266, {{3, 3, 143, 286}});
    single(1, 1, 48, 48, 105, 100, 10, 10, {{1, 1, 0, -1}, {1, 2, 0, -1}, {2, 1, 0, -1}});
    CHECK(tplsyn::div_trunc_pow2(-500, 8) == -1 && tplsyn::div_trunc_pow2(-256, 8) == -1 && tplsyn::div_trunc_pow2(-255, 8) == 0 && tplsyn::div_trunc_pow2(511, 8) == 1);
    CHECK(tplsyn::round_floor(-1, 16) == -1 && tplsyn::round_floor(-16, 16) == -1 && tplsyn::round_floor(-17, 16) == -2 && tplsyn::round_floor(15, 16) == 0);
    // GET_MV_RAWPEL rounds to the nearest whole sample, halves away from zero
    CHECK(tplsyn::mv_rawpel(43) == 5 && tplsyn::mv_rawpel(44) == 6 && tplsyn::mv_rawpel(-21) == -3 && tplsyn::mv_rawpel(-20) == -3 && tplsyn::mv_rawpel(-19) == -2);
    CHECK(tplsyn::mv_rawpel(3) == 0 && tplsyn::mv_rawpel(4) == 1 && tplsyn::mv_rawpel(-3) == 0 && tplsyn::mv_rawpel(-4) == -1);
}

// file: int32 w, h, cell_log2, sb_size, base_rdmult, n; double r0_in; per picture int32 on, ref_window[8], then its records; then the expected grids and output
bool read(std::FILE* f, void* dst, size_t n) { return std::fread(dst, 1, n, f) == n; }
void from_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); failures++; return; }
    int32_t hd[6];
    double r0_in;
    CHECK(read(f, hd, sizeof hd) && read(f, &r0_in, sizeof r0_in));
    Window W(hd[0], hd[1], hd[2], hd[3], hd[4], r0_in, hd[5]);
    for (int i = 0; i < hd[5]; i++) {
        int32_t fr[9];
        CHECK(read(f, fr, sizeof fr) && read(f, W.stats[i], W.n_mb * sizeof(SvtHipTplMbStats)));
        W.frames[i].on = fr[0];
        for (int k = 0; k < 8; k++) W.frames[i].ref_window[k] = fr[1 + k];
    }
    CHECK(W.run());
    std::vector<char> want(W.dep_bytes > W.out_bytes ? W.dep_bytes : W.out_bytes);
    for (int i = 0; i < hd[5]; i++) {
        CHECK(read(f, want.data(), W.dep_bytes));
        CHECK(std::memcmp(want.data(), W.dep[i], W.dep_bytes) == 0);
    }
    CHECK(read(f, want.data(), W.out_bytes));
    CHECK(std::memcmp(want.data(), W.out, W.out_bytes) == 0);
    std::fclose(f);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1) from_file(argv[1]);
    else closed_forms();
    if (failures) return 1;
    std::printf("ok %s\n", argc > 1 ? "window" : "closed forms");
    return 0;
}
