// ibc_search.hip — svt_av1_full_pixel_search of the intra-block-copy path for a list of blocks on gfx950 (wave64), behind svt_hip_ibc_full_search_batch_dev: the
// diamond search with its refinement, the mesh search, the hash search of ibc_hash.hip and the choice between the three.
//
// Replaces (file:line under Source/Lib of the reference):
//   Encoder/Codec/av1me.c:437-573, :578-643, :712-775    svt_av1_diamond_search_sad_c, full_pixel_diamond, svt_av1_refining_search_sad
//   Encoder/Codec/av1me.c:346-435, :650-710              exhuastive_mesh_search, full_pixel_exhaustive
//   Encoder/Codec/av1me.c:1306-1411                      case NSTEP of svt_av1_full_pixel_search and its hash tail
//   Encoder/Codec/EbModeDecision.c:4523                  av1_is_dv_valid of the final vector
// The walks themselves are ibc_search.h, the same text the host form runs: here every lane of a wave runs a walk with the same values, and the evaluator takes a
// block's sums across the lanes (small blocks: several sites of a step side by side, a group of lanes each).
//
// Launches, the same number whatever the data:
//   ibc_diamond_kernel     a workgroup of four waves per job.  The passes of full_pixel_diamond all start from the same clamped point, so each wave walks the
//                          passes p = wave, wave + 4, ..., all 11 - step_param of them; wave 0 then replays the reference's bookkeeping (n, num00, do_refine)
//                          over the finished passes, runs the refinement, compares with the threshold and leaves the mesh walk's first state in d_scratch.
//   ibc_mesh_kernel        x MAX_MESH_STEP, a workgroup per (job, strip of candidate rows); a job whose walk does not run, or has ended, leaves at once.  The
//                          block is in LDS; a thread takes a candidate, neighbouring lanes neighbouring columns, and keeps the smallest (total, scan index).  The
//                          strips' minima go to d_scratch; nothing depends on the order of arrival and no atomic decides a winner.  The candidates' samples are
//                          read from global memory (no LDS window yet: docs/kernels/ibc_hash.md).
//   ibc_mesh_reduce_kernel x MAX_MESH_STEP, a wave per job: the centre's total (scan index 0), the smallest of the strips' minima, the next scan's centre and
//                          pattern; after the walk's last scan the variance of the winner.
//   ibc_search_kernel      of ibc_hash.hip, unchanged, on a job list the diamond kernel derives (a job the hash tail does not apply to gets block_size 0 there,
//                          which that kernel answers with count = -1); not launched without a table.
//   ibc_choose_kernel      a thread per job: the two comparisons and dv_valid.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svt_hip_internal.h"
#include "fmt_dispatch.h"
#include "lane_reduce.h"
#include "ibc_search.h"

namespace {

#define PD __device__ __forceinline__

constexpr int WG = 256, WAVES = WG / 64;
static_assert(ibcs::MESH_STRIPS == 64, "the reduce kernel reads a strip a lane");

struct Patterns {
    int32_t v[2 * ibcs::MAX_MESH_STEP];
};

// the sums of a block_w x block_h block against its displaced copies, by a whole wave: every lane calls with the same arguments and gets the same result
template <class PIX, int BD> struct WaveEval {
    const PIX* what;   // the block's top-left sample
    int        stride, bw, bw_log2, n, lane;
    PD uint32_t diff_at(const PIX* cand, int k) const {
        const ptrdiff_t o = (ptrdiff_t)(k >> bw_log2) * stride + (k & (bw - 1));
        return (uint32_t)abs((int)what[o] - (int)cand[o]);
    }
    PD uint32_t sad(int row, int col) const {
        const PIX* cand = what + (ptrdiff_t)row * stride + col;
        uint32_t   s = 0;   // at most 256 samples a lane
        for (int k = lane; k < n; k += 64) s += diff_at(cand, k);
        return wave_sum_u32(s);
    }
    PD void sads(uint32_t rows, uint32_t cols, int cnt, int centre_row, int centre_col, int len, unsigned mask, uint32_t* out) const {
        if (n >= 64) {
            for (int j = 0; j < cnt; ++j) out[j] = (mask >> j) & 1 ? sad(centre_row + len * ibcs::unpack(rows, j), centre_col + len * ibcs::unpack(cols, j)) : 0;
            return;
        }
        // 16 or 32 samples: 4 or 2 sites side by side, a group of n lanes each, a lane a sample
        const int per = 64 / n, g = lane / n, k = lane & (n - 1);
        for (int base = 0; base < cnt; base += per) {
            const int j = base + g;
            uint32_t  v = 0;
            if (j < cnt && ((mask >> j) & 1)) v = diff_at(what + (ptrdiff_t)(centre_row + len * ibcs::unpack(rows, j)) * stride + (centre_col + len * ibcs::unpack(cols, j)), k);
            for (int m = 1; m < n; m <<= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
            for (int t = 0; t < per && base + t < cnt; ++t) out[base + t] = (uint32_t)__shfl((int)v, t * n, 64);
        }
    }
    PD uint32_t var(int row, int col) const {
        const PIX* cand = what + (ptrdiff_t)row * stride + col;
        int        sum = 0;   // at most 256 samples a lane: |sum| <= 256 * 1023, sse <= 256 * 1023^2 < 2^32
        uint32_t   sse = 0;
        for (int k = lane; k < n; k += 64) {
            const ptrdiff_t o = (ptrdiff_t)(k >> bw_log2) * stride + (k & (bw - 1));
            const int       d = (int)what[o] - (int)cand[o];
            sum += d;
            sse += (uint32_t)(d * d);
        }
        return ibcs::variance_wh(wave_sum_i64((long long)sum), wave_sum_u64((unsigned long long)sse), n, BD);
    }
};
template <class PIX, int BD> PD WaveEval<PIX, BD> wave_eval(const PIX* luma, int stride, const ibcs::Job& J, int lane) {
    return WaveEval<PIX, BD>{luma + (size_t)J.y_pos * stride + J.x_pos, stride, J.block_w, ibcs::ilog2(J.block_w), J.block_w * J.block_h, lane};
}
PD uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = min(v, lane_xor(v, m));
    return v;
}
static_assert(sizeof(ibcs::Job) % 4 == 0 && sizeof(ibcs::Job) / 4 <= 64, "copied by words by one wave");
PD void load_job(ibcs::Job* dst, const ibcs::Job* src, int tid) {
    if (tid < (int)(sizeof(ibcs::Job) / 4)) ((uint32_t*)dst)[tid] = ((const uint32_t*)src)[tid];
}

template <class PIX, int BD> __global__ __launch_bounds__(WG) void ibc_diamond_kernel(const PIX* __restrict__ luma, int stride, int width, int height, int have_tables,
                                                                                      const int32_t* __restrict__ jc, const int32_t* __restrict__ cc, Patterns pat,
                                                                                      const ibcs::Job* __restrict__ jobs, ibcs::Result* __restrict__ results,
                                                                                      ibcs::MeshState* __restrict__ states, SvtHipIbcSearchJob* __restrict__ hash_jobs) {
    __shared__ ibcs::Job  s_job;
    __shared__ ibcs::Pass s_pass[ibcs::MAX_MVSEARCH_STEPS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, job = blockIdx.x;
    load_job(&s_job, jobs + job, tid);
    __syncthreads();
    const ibcs::Job J = s_job;
    const int       status = ibcs::job_status(J, width, height, have_tables != 0);   // the same for every thread
    if (status) {
        if (tid == 0) {
            results[job] = ibcs::empty_full_result(status);
            states[job] = ibcs::MeshState{};
            hash_jobs[job] = ibcs::hash_job(J, false);
        }
        return;
    }
    const WaveEval<PIX, BD> ev = wave_eval<PIX, BD>(luma, stride, J, lane);
    const int               npass = ibcs::MAX_MVSEARCH_STEPS - J.step_param;
    for (int p = wave; p < npass; p += WAVES) {
        const ibcs::Pass r = ibcs::diamond_pass(ev, J, J.step_param + p, jc, cc);
        if (lane == 0) s_pass[p] = r;
    }
    __syncthreads();
    if (wave) return;
    const ibcs::Diamond d = ibcs::full_pixel_diamond(ev, J, [&](int n) { return s_pass[n]; }, jc, cc);
    if (lane) return;
    ibcs::Result    R = ibcs::empty_full_result(0);
    ibcs::MeshState s{};
    ibcs::set_diamond(R, d);
    if (J.exhaustive_allowed && d.var > ibcs::exhaustive_thr(J)) {
        R.mesh_ran = 1;
        s = ibcs::mesh_begin(pat.v, d.row, d.col);
    }
    results[job] = R;
    states[job] = s;
    hash_jobs[job] = ibcs::hash_job(J, ibcs::hash_applies(J));
}

// one scan of one strip of candidate rows of one job
template <class PIX> __global__ __launch_bounds__(WG) void ibc_mesh_kernel(const PIX* __restrict__ luma, int stride, const int32_t* __restrict__ jc,
                                                                           const int32_t* __restrict__ cc, const ibcs::Job* __restrict__ jobs,
                                                                           const ibcs::MeshState* __restrict__ states, uint64_t* __restrict__ partial) {
    __shared__ ibcs::Job s_job;
    __shared__ uint16_t  s_what[128 * 128];
    __shared__ uint64_t  s_min[WAVES];
    const int             tid = threadIdx.x, job = blockIdx.x / ibcs::MESH_STRIPS, strip = blockIdx.x % ibcs::MESH_STRIPS;
    const ibcs::MeshState s = states[job];
    if (!s.run) return;   // the same for every thread
    load_job(&s_job, jobs + job, tid);
    __syncthreads();
    const ibcs::Job      J = s_job;
    const ibcs::MeshGeom g = ibcs::mesh_geom(J, s.row, s.col, s.range, s.step);
    const int            rows_per = (g.nrows + ibcs::MESH_STRIPS - 1) / ibcs::MESH_STRIPS, i0 = strip * rows_per, i1 = min(g.nrows, i0 + rows_per);
    if (i0 >= i1 || g.ncols == 0) {
        if (tid == 0) partial[(size_t)job * ibcs::MESH_STRIPS + strip] = UINT64_MAX;
        return;
    }
    const int  bw = J.block_w, bh = J.block_h, n = bw * bh, bw_log2 = ibcs::ilog2(bw);
    const PIX* what = luma + (size_t)J.y_pos * stride + J.x_pos;
    for (int k = tid; k < n; k += WG) s_what[k] = (uint16_t)what[(size_t)(k >> bw_log2) * stride + (k & (bw - 1))];
    __syncthreads();
    uint64_t  best = UINT64_MAX;
    const int total = (i1 - i0) * g.ncols;   // at most 9 * 513
    for (int idx = tid; idx < total; idx += WG) {
        const int  i = i0 + idx / g.ncols, k = idx % g.ncols;
        const int  row = g.centre_row + g.start_row + i * g.step, col = g.centre_col + g.start_col + k * g.col_stride;
        const PIX* cand = what + (ptrdiff_t)row * stride + col;
        uint32_t   sad = 0;
        for (int y = 0; y < bh; ++y) {
            const PIX*      c = cand + (ptrdiff_t)y * stride;
            const uint16_t* w = s_what + y * bw;
            for (int x = 0; x < bw; x += 4)   // every width is a multiple of 4
                sad += (uint32_t)abs((int)w[x] - (int)c[x]) + (uint32_t)abs((int)w[x + 1] - (int)c[x + 1]) + (uint32_t)abs((int)w[x + 2] - (int)c[x + 2]) +
                       (uint32_t)abs((int)w[x + 3] - (int)c[x + 3]);
        }
        best = min(best, ibcs::mesh_key(sad + ibcs::mvsad_err_cost(J, row, col, jc, cc), 1u + (uint32_t)(i * g.ncols + k)));
    }
    best = wave_min_u64(best);
    if ((tid & 63) == 0) s_min[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) partial[(size_t)job * ibcs::MESH_STRIPS + strip] = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
}

// a wave per job: the scan's winner, the walk's next state, and after the last scan the winner's variance
template <class PIX, int BD> __global__ __launch_bounds__(64) void ibc_mesh_reduce_kernel(const PIX* __restrict__ luma, int stride, const int32_t* __restrict__ jc,
                                                                                          const int32_t* __restrict__ cc, Patterns pat, const ibcs::Job* __restrict__ jobs,
                                                                                          ibcs::MeshState* __restrict__ states, const uint64_t* __restrict__ partial,
                                                                                          ibcs::Result* __restrict__ results) {
    __shared__ ibcs::Job s_job;
    const int       lane = threadIdx.x, job = blockIdx.x;
    ibcs::MeshState s = states[job];
    if (!s.run) return;
    load_job(&s_job, jobs + job, lane);
    __syncthreads();
    const ibcs::Job         J = s_job;
    const WaveEval<PIX, BD> ev = wave_eval<PIX, BD>(luma, stride, J, lane);
    const ibcs::MeshGeom    g = ibcs::mesh_geom(J, s.row, s.col, s.range, s.step);
    const uint64_t          centre = ibcs::mesh_key(ev.sad(g.centre_row, g.centre_col) + ibcs::mvsad_err_cost(J, g.centre_row, g.centre_col, jc, cc), 0);
    const uint64_t          key = wave_min_u64(min(centre, partial[(size_t)job * ibcs::MESH_STRIPS + lane]));
    int                     row, col;
    ibcs::mesh_decode(g, key, &row, &col);
    ibcs::mesh_advance(s, pat.v, (uint32_t)(key >> 32), row, col);
    int var = s.best;
    if (!s.run && s.best < INT32_MAX) var = ibcs::pred_var(ev, J, row, col, jc, cc);
    if (lane) return;
    states[job] = s;
    if (s.run) return;
    results[job].mesh_passes = s.passes;
    results[job].mesh_var = var;
    results[job].mesh_row = row;
    results[job].mesh_col = col;
}

__global__ __launch_bounds__(WG) void ibc_choose_kernel(const ibcs::Job* __restrict__ jobs, int njobs, const SvtHipIbcSearchResult* __restrict__ hash_results,
                                                        ibcs::Result* __restrict__ results) {
    const int job = blockIdx.x * WG + threadIdx.x;
    if (job >= njobs) return;
    ibcs::Result R = results[job];
    if (R.status) return;
    const ibcs::Job J = jobs[job];
    if (hash_results && ibcs::hash_applies(J)) {
        const SvtHipIbcSearchResult h = hash_results[job];
        if (h.count >= 0) R.hash = h;
    }
    ibcs::choose(R, J);
    results[job] = R;
}

}  // namespace

int svt_hip_launch_ibc_full_search(hipStream_t st, int pix_bytes, int bd, const void* luma, int stride, int width, int height, const int32_t* bucket_start,
                                   const SvtHipIbcHashEntry* entries, const int32_t* joint_cost, const int32_t* comp_cost, const int32_t* mesh_patterns,
                                   const SvtHipIbcFullSearchJob* jobs, int njobs, SvtHipIbcFullSearchResult* results, void* scratch) {
    const ibcs::FullScratch L = ibcs::full_scratch(njobs);
    ibcs::MeshState*        states = (ibcs::MeshState*)((uint8_t*)scratch + L.state);
    uint64_t*               partial = (uint64_t*)((uint8_t*)scratch + L.partial);
    SvtHipIbcSearchJob*     hash_jobs = (SvtHipIbcSearchJob*)((uint8_t*)scratch + L.hash_jobs);
    SvtHipIbcSearchResult*  hash_results = bucket_start ? (SvtHipIbcSearchResult*)((uint8_t*)scratch + L.hash_results) : nullptr;
    Patterns                pat;
    for (int i = 0; i < 2 * ibcs::MAX_MESH_STEP; ++i) pat.v[i] = mesh_patterns[i];
    svt_for_fmt(pix_bytes, bd, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        constexpr int BD = decltype(f)::bd;
        hipLaunchKernelGGL((ibc_diamond_kernel<PIX, BD>), dim3(njobs), dim3(WG), 0, st, (const PIX*)luma, stride, width, height, bucket_start ? 1 : 0, joint_cost, comp_cost, pat,
                           jobs, results, states, hash_jobs);
        for (int pass = 0; pass < ibcs::MAX_MESH_STEP; ++pass) {
            hipLaunchKernelGGL((ibc_mesh_kernel<PIX>), dim3((unsigned)njobs * ibcs::MESH_STRIPS), dim3(WG), 0, st, (const PIX*)luma, stride, joint_cost, comp_cost, jobs,
                               (const ibcs::MeshState*)states, partial);
            hipLaunchKernelGGL((ibc_mesh_reduce_kernel<PIX, BD>), dim3(njobs), dim3(64), 0, st, (const PIX*)luma, stride, joint_cost, comp_cost, pat, jobs, states,
                               (const uint64_t*)partial, results);
        }
    });
    int rc = (int)hipGetLastError();
    if (rc != (int)hipSuccess) return rc;
    if (bucket_start) {
        rc = svt_hip_launch_ibc_hash_search(st, pix_bytes, bd, luma, stride, width, height, bucket_start, entries, joint_cost, comp_cost, hash_jobs, njobs, hash_results);
        if (rc != (int)hipSuccess) return rc;
    }
    hipLaunchKernelGGL(ibc_choose_kernel, dim3((njobs + WG - 1) / WG), dim3(WG), 0, st, jobs, njobs, (const SvtHipIbcSearchResult*)hash_results, results);
    return (int)hipGetLastError();
}

SVT_HIP_TU_PROBE(ibc_search)
