// tpl_synth.hip — the look-ahead's TPL flow synthesizer and generate_r0beta on the device; gfx950 (wave64).
//
// Replaces (file:line under Source/Lib of the reference; the arithmetic itself is tpl_synth.h, shared with the host form):
//   Encoder/Codec/EbRateControlProcess.c:887-998     tpl_mc_flow_synthesizer -> tpl_model_update -> tpl_model_update_b for one picture of the window
//   Encoder/Codec/EbRateControlProcess.c:1000-1075   generate_r0beta, :39-84 generate_lambda_scaling_factor
//
// Scatter, one launch per window picture: one thread per source block = per cell of the picture's grid (a macroblock, or a quarter when cells are 8x8),
// consecutive lanes = consecutive cells of a grid row.  The thread reads its macroblock's record and its own cell and adds into the up to four cells of the
// target picture's grid with 64-bit atomic adds (two's complement: the reference's accumulators are int64_t and integer adds commute, so any order gives
// the reference's sums).  Zero addends are skipped.  The pictures of a window are ordered by the stream: picture k's launch reads what the launches of
// k + 1 .. n - 1 added to its grid.  Inside one launch a cell is read only by its own thread, and written only when the picture is its own target through
// ref_window[0] -- then by that same thread, after its read (the zero vector's only non-zero overlap is the block's own cell).
// r0 / beta / factors, two launches: the two int64 base sums go through a wave sum and an LDS sum into one atomic per workgroup each; the second launch
// divides them into r0 (every thread the same IEEE division) and writes a macroblock's factor or a superblock's beta per thread, the double sums of a
// macroblock's <= 4 terms inside the thread in the reference's order.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "svt_hip_internal.h"
#include "lane_reduce.h"
#include "tpl_synth.h"

namespace {

using namespace tplsyn;

constexpr int SYNTH_THREADS = 256;

struct SynthArgs {
    Geom g;
    const SvtHipTplMbStats* stats;
    const int64_t* own;
    int64_t* target[8];   // [rf_idx + 1], NULL = not in the window
};

__device__ __forceinline__ void add64(int64_t* p, int64_t v) {
    if (v) atomicAdd((unsigned long long*)p, (unsigned long long)v);
}

__global__ __launch_bounds__(SYNTH_THREADS) void tpl_synth_kernel(const SynthArgs A) {
    const int idx = blockIdx.x * SYNTH_THREADS + threadIdx.x;
    if (idx >= A.g.rows * A.g.cols) return;
    const int row = idx / A.g.cols, col = idx - row * A.g.cols;
    const SvtHipTplMbStats rec = A.stats[(row >> A.g.s) * A.g.mb_cols + (col >> A.g.s)];
    const Block b = block_of(A.g, rec, A.own[2 * (size_t)idx], A.own[2 * (size_t)idx + 1], row, col);
    if (b.slot < 0) return;
    // slot b.slot of the kernel argument, read from the kernel-argument segment itself: an index into the by-value copy would move it to private memory
    // (the argument is the kernel's only one: offset 0)
    int64_t* const* targets = (int64_t* const*)((const char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(SynthArgs, target));
    int64_t* t = targets[b.slot];
    if (!t) return;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int cell;
        int64_t add_rate, add_dist;
        if (!target_of(A.g, b, k, &cell, &add_rate, &add_dist)) continue;
        add64(t + 2 * (size_t)cell, add_rate);
        add64(t + 2 * (size_t)cell + 1, add_dist);
    }
}

struct R0Args {
    Geom g;
    int sb_size, sb_cols, sb_rows;
    int32_t rm;
    double r0_in;
    const SvtHipTplMbStats* stats;
    const int64_t* dep;
    unsigned long long* sums;   // {intra_cost_base, mc_dep_cost_base}, zero before the first launch
    void* out;
};

__global__ __launch_bounds__(SYNTH_THREADS) void tpl_base_sums_kernel(const R0Args A) {
    __shared__ unsigned long long part[SYNTH_THREADS / 64][2];
    const int idx = blockIdx.x * SYNTH_THREADS + threadIdx.x;
    unsigned long long intra = 0, mc = 0;
    if (idx < A.g.rows * A.g.cols) {
        const int row = idx / A.g.cols, col = idx - row * A.g.cols;
        if (base_has_row(A.g, row)) {
            intra = (unsigned long long)cell_intra(cell_recrf(A.g, A.stats, row, col));
            mc = intra + (unsigned long long)cell_delta(A.g, A.rm, A.dep, row, col);
        }
    }
    intra = wave_sum_u64(intra); mc = wave_sum_u64(mc);
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6][0] = intra; part[threadIdx.x >> 6][1] = mc; }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long v = 0;
#pragma unroll
        for (int i = 0; i < SYNTH_THREADS / 64; i++) v += part[i][threadIdx.x];
        if (v) atomicAdd(A.sums + threadIdx.x, v);
    }
}

__global__ __launch_bounds__(SYNTH_THREADS) void tpl_factor_beta_kernel(const R0Args A) {
    const int idx = blockIdx.x * SYNTH_THREADS + threadIdx.x;
    const int n_mb = A.g.mb_cols * A.g.mb_rows, n_sb = A.sb_cols * A.sb_rows;
    if (idx >= n_mb + n_sb) return;
    const int64_t intra_base = (int64_t)A.sums[0], mc_base = (int64_t)A.sums[1];
    const double r0 = r0_of(A.r0_in, intra_base, mc_base);
    SvtHipTplR0BetaHeader* hd = (SvtHipTplR0BetaHeader*)A.out;
    double* factors = (double*)(hd + 1);
    if (idx == 0) { hd->r0 = r0; hd->intra_cost_base = intra_base; hd->mc_dep_cost_base = mc_base; }
    if (idx < n_mb) {
        const int r = idx / A.g.mb_cols;
        factors[idx] = factor_of(A.g, A.rm, A.stats, A.dep, r, idx - r * A.g.mb_cols, mc_base, r0);
    } else {
        const int k = idx - n_mb, r = k / A.sb_cols;
        factors[idx] = beta_of(A.g, A.sb_size, A.rm, A.stats, A.dep, r, k - r * A.sb_cols, r0);   // beta[] follows factors[n_mb]
    }
}

}  // namespace

extern "C" int svt_hip_launch_tpl_synth(hipStream_t st, int w, int h, int cell_log2, const SvtHipTplMbStats* stats, const int64_t* own, int64_t* const target[8]) {
    SynthArgs A = {};
    A.g = geom(w, h, cell_log2);
    A.stats = stats; A.own = own;
    bool any = false;
    for (int k = 0; k < 8; k++) { A.target[k] = target[k]; any |= target[k] != nullptr; }
    const int n = A.g.rows * A.g.cols;
    if (!any || n <= 0) return 0;
    hipLaunchKernelGGL(tpl_synth_kernel, dim3((n + SYNTH_THREADS - 1) / SYNTH_THREADS), dim3(SYNTH_THREADS), 0, st, A);
    return (int)hipGetLastError();
}

extern "C" int svt_hip_launch_tpl_r0beta(hipStream_t st, const SvtHipTplSynthParams* p, const SvtHipTplMbStats* stats, const int64_t* dep, void* out, void* scratch) {
    R0Args A = {};
    A.g = geom(p->w, p->h, p->cell_log2);
    A.sb_size = p->sb_size; A.sb_cols = sb_count(p->w, p->sb_size); A.sb_rows = sb_count(p->h, p->sb_size);
    A.rm = p->base_rdmult; A.r0_in = p->r0_in;
    A.stats = stats; A.dep = dep; A.sums = (unsigned long long*)scratch; A.out = out;
    if (hipError_t e = hipMemsetAsync(scratch, 0, 2 * sizeof(unsigned long long), st)) return (int)e;
    const int n = A.g.rows * A.g.cols, m = A.g.mb_cols * A.g.mb_rows + A.sb_cols * A.sb_rows;
    hipLaunchKernelGGL(tpl_base_sums_kernel, dim3((n + SYNTH_THREADS - 1) / SYNTH_THREADS), dim3(SYNTH_THREADS), 0, st, A);
    hipLaunchKernelGGL(tpl_factor_beta_kernel, dim3((m + SYNTH_THREADS - 1) / SYNTH_THREADS), dim3(SYNTH_THREADS), 0, st, A);
    return (int)hipGetLastError();
}

SVT_HIP_TU_PROBE(tpl_synth)
