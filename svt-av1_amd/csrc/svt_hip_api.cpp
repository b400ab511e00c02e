// svt_hip_api.cpp — the C-ABI layer of libsvtav1_hip.so (include/svt_hip.h): context, memory,
// host-pointer convenience wrappers around the batched kernel launchers.
#include <hip/hip_runtime.h>
#include <math.h>
#include <limits.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "svt_hip_internal.h"
#include "svt_hip_host.h"
#include "tpl_synth.h"
#include "resize_plan.h"
#include "ibc_hash.h"
#include "ibc_search.h"
#include "scaled_pred.h"
#include "comp_search.h"
#include "obmc_search.h"
#include "ifs_search.h"
#include <mutex>

struct SvtHipCtx {
    int         device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t  ev0 = nullptr, ev1 = nullptr;
    int         select_form = -1;   // svt_hip_set_cdef_select_form
    hipEvent_t  ev_sel_in = nullptr, ev_sel_out = nullptr;   // hand-over to and from the device's selection stream (svt_hip_cdef_strength_select_dev)
    int         tpl_phases = 7;     // svt_hip_tpl_set_phases
    int         me_waves = 4;   // 256 threads per SB: measured best on MI355X (tools/me_time.py)
    int         me_big = 1;     // also launch the strip-walking instance for search areas above 65 536 candidates
    void*       scratch = nullptr;   // library-owned device scratch (16-bit Wiener statistics, self-guided unit search), grown on demand
    size_t      scratch_bytes = 0;
    void*       host_scratch = nullptr;   // pinned host staging of the self-guided unit search
    size_t      host_scratch_bytes = 0;
    void*       me_buf = nullptr;         // device staging of svt_hip_me_fullpel_frame (host-pointer form), grown on demand
    size_t      me_buf_bytes = 0;
    uint16_t*   gm_lut = nullptr;         // device copy of the global-motion error table, made by the first global-motion call
    uint8_t*    wedge_masks = nullptr;    // device copy of the wedge mask table (comp_search.h), made by the first call that needs it
    void*       rd_grids = nullptr;       // device copy of the tables of svt_hip_set_rd_curvfit_grids: rate[4][65], dist[2][65] as double, then cat[22] as int32
    bool        rd_grids_set = false;
    void*       comp_jobs = nullptr;      // device staging of svt_hip_compound_search_batch_dev's job list, grown on demand
    size_t      comp_jobs_bytes = 0;
    void*       job_stage[3] = {nullptr, nullptr, nullptr};   // device staging of the job lists of svt_hip_obmc_target_batch_dev [0], svt_hip_obmc_search_batch_dev [1]
    size_t      job_stage_bytes[3] = {0, 0, 0};               // and svt_hip_ifs_search_batch_dev [2], each grown on demand
    std::string err;
};

namespace {
int fail(SvtHipCtx* c, hipError_t e, const char* what) {
    if (c) c->err = std::string(what) + ": " + hipGetErrorString(e);
    return SVT_HIP_ERR_RUNTIME;
}
// An entry point is three lines (docs/design/kernels-overview.md):
//     SVT_HIP_ENTER(c);
//     if (!c || <what it refuses>) return bad_arg(c, "svt_hip_x_dev: bad argument");
//     return launched(c, svt_hip_launch_x(c->stream, ...), "x launch");
// A refusal's text is a literal at its call site.  It is left out where the caller is the per-call table of rtcd_hip.cpp and the refusal only says "not this
// entry point's domain": the table tells a delegation (the context's text is as it was) from a device failure (there is a text) by exactly that.
int bad_arg(SvtHipCtx* c, const char* msg = nullptr) {
    if (c && msg) c->err = msg;
    return SVT_HIP_ERR_BAD_ARG;
}
int launched(SvtHipCtx* c, int rc, const char* what) { return rc == hipSuccess ? SVT_HIP_OK : fail(c, (hipError_t)rc, what); }
// 8-bit samples in bytes, 8- or 10-bit samples in 16-bit words
bool fmt_ok(int pix_bytes, int bd) { return (pix_bytes == 1 || pix_bytes == 2) && (bd == 8 || bd == 10) && !(pix_bytes == 1 && bd != 8); }
// the sample size alone (entry points whose kernels take no bit depth, or take it as a value)
bool pix_ok(int pix_bytes) { return pix_bytes == 1 || pix_bytes == 2; }
// ... 8-, 10- or 12-bit samples in 16-bit words: the kernels with a 12-bit instance
bool fmt12_ok(int pix_bytes, int bd) { return (pix_bytes == 1 && bd == 8) || (pix_bytes == 2 && (bd == 8 || bd == 10 || bd == 12)); }
// ... any depth from 8 to 12 in 16-bit words (9 and 11 too): the kernels that take the bit depth as a value
bool fmt_8to12_ok(int pix_bytes, int bd) { return (pix_bytes == 1 && bd == 8) || (pix_bytes == 2 && bd >= 8 && bd <= 12); }
}  // namespace
#define HIPCHK(c, call)                                   \
    do {                                                  \
        hipError_t e_ = (call);                           \
        if (e_ != hipSuccess) return fail((c), e_, #call); \
    } while (0)

// Every entry point makes the context's device current first: one encoder process may drive several GPUs, each from its own host thread
// ("host worker i owns GPU i"); hipSetDevice is a thread-local switch.
#define SVT_HIP_ENTER(c)                                                              \
    do {                                                                              \
        if ((c) && hipSetDevice((c)->device) != hipSuccess) return SVT_HIP_ERR_RUNTIME; \
    } while (0)

// The one-launch CDEF strength selection keeps 256 workgroups resident that wait for each other; two such launches on different streams could each hold a
// part of the compute units and wait for the rest forever.  Every context of a device therefore issues them on ONE stream of that device (created with the
// first context, kept for the life of the process), ordered against the caller's stream with a pair of events; kernels that do not wait for other workgroups
// run beside it as before.  Works under stream capture too (the event wait pulls the selection stream into the capture, the second event joins it back).
// While the caller's stream is being captured the order is expressed inside the capture instead: each captured selection waits for the event the previous
// captured selection of the same capture recorded (a fresh event per call; they are kept until the process ends, a graph may be instantiated from them later),
// so the selection nodes of a graph's parallel branches form one chain.
static std::mutex  g_sel_mutex;
static hipStream_t g_sel_stream[64];
static hipEvent_t  g_sel_cap_event[64];
static unsigned long long g_sel_cap_id[64];
extern "C" int svt_hip_strength_select_is_resident(int form, int sb_count);

extern "C" {

int svt_hip_init(int device_id, SvtHipCtx** out) {
    if (!out) return SVT_HIP_ERR_BAD_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) return SVT_HIP_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return SVT_HIP_ERR_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        std::fprintf(stderr, "svt_hip_init: device %d is %s; this library is built for gfx950 only\n", device_id,
                     prop.gcnArchName);
        return SVT_HIP_ERR_NO_DEVICE;
    }
    SvtHipCtx* c = new SvtHipCtx();
    c->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess || hipStreamCreate(&c->own_stream) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_sel_in, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->ev_sel_out, hipEventDisableTiming) != hipSuccess) {
        delete c;
        return SVT_HIP_ERR_RUNTIME;
    }
    if (device_id < 64) {
        std::lock_guard<std::mutex> lk(g_sel_mutex);
        if (!g_sel_stream[device_id] && hipStreamCreateWithFlags(&g_sel_stream[device_id], hipStreamNonBlocking) != hipSuccess) g_sel_stream[device_id] = nullptr;
    }
    c->stream = c->own_stream;
    *out = c;
    return SVT_HIP_OK;
}

void svt_hip_destroy(SvtHipCtx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->ev_sel_in) (void)hipEventDestroy(c->ev_sel_in);
    if (c->ev_sel_out) (void)hipEventDestroy(c->ev_sel_out);
    if (c->scratch) (void)hipFree(c->scratch);
    if (c->host_scratch) (void)hipHostFree(c->host_scratch);
    if (c->me_buf) (void)hipFree(c->me_buf);
    if (c->gm_lut) (void)hipFree(c->gm_lut);
    if (c->wedge_masks) (void)hipFree(c->wedge_masks);
    if (c->rd_grids) (void)hipFree(c->rd_grids);
    if (c->comp_jobs) (void)hipFree(c->comp_jobs);
    for (void* p : c->job_stage)
        if (p) (void)hipFree(p);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

const char* svt_hip_last_error(const SvtHipCtx* c) { return c ? c->err.c_str() : "null context"; }

int svt_hip_set_stream(SvtHipCtx* c, void* s) {
    SVT_HIP_ENTER(c);
    if (!c) return bad_arg(c);
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return SVT_HIP_OK;
}
void* svt_hip_ctx_stream(SvtHipCtx* c) { return c ? (void*)c->stream : nullptr; }
int   svt_hip_ctx_device(SvtHipCtx* c) { return c ? c->device : 0; }
void  svt_hip_ctx_clear_error(SvtHipCtx* c) { if (c) c->err.clear(); }
int svt_hip_sync(SvtHipCtx* c) {
    SVT_HIP_ENTER(c);
    if (!c) return bad_arg(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SVT_HIP_OK;
}
int svt_hip_malloc(SvtHipCtx* c, void** p, size_t bytes) {
    SVT_HIP_ENTER(c);
    if (!c || !p) return bad_arg(c);
    HIPCHK(c, hipMalloc(p, bytes ? bytes : 4));
    return SVT_HIP_OK;
}
int svt_hip_free(SvtHipCtx* c, void* p) {
    SVT_HIP_ENTER(c);
    if (!c) return bad_arg(c);
    HIPCHK(c, hipFree(p));
    return SVT_HIP_OK;
}
// Copies are ordered on the context's stream; the forms without _async in their name hand over only after the stream has drained.
static int copy_1d(SvtHipCtx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind, bool sync) {
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, kind, c->stream));
    if (sync) HIPCHK(c, hipStreamSynchronize(c->stream));
    return SVT_HIP_OK;
}
static int copy_2d(SvtHipCtx* c, void* dst, size_t dpitch, const void* src, size_t spitch, size_t wbytes, size_t rows, hipMemcpyKind kind, bool sync) {
    HIPCHK(c, hipMemcpy2DAsync(dst, dpitch, src, spitch, wbytes, rows, kind, c->stream));
    if (sync) HIPCHK(c, hipStreamSynchronize(c->stream));
    return SVT_HIP_OK;
}
int svt_hip_memcpy_h2d(SvtHipCtx* c, void* d, const void* h, size_t bytes) {
    SVT_HIP_ENTER(c);
    if (!c) return bad_arg(c);
    return copy_1d(c, d, h, bytes, hipMemcpyHostToDevice, true);
}
int svt_hip_memcpy_d2h(SvtHipCtx* c, void* h, const void* d, size_t bytes) {
    SVT_HIP_ENTER(c);
    if (!c) return bad_arg(c);
    return copy_1d(c, h, d, bytes, hipMemcpyDeviceToHost, true);
}
int svt_hip_memcpy_d2d(SvtHipCtx* c, void* dst, const void* src, size_t bytes) {   // asynchronous, ordered on the context's stream
    if (!c || (!dst && bytes) || (!src && bytes)) return bad_arg(c);
    if (!bytes) return SVT_HIP_OK;
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    return SVT_HIP_OK;
}
int svt_hip_memcpy2d_h2d(SvtHipCtx* c, void* d, size_t dpitch, const void* h, size_t hpitch, size_t wbytes, size_t rows) {
    SVT_HIP_ENTER(c);
    if (!c || !d || !h || dpitch < wbytes || hpitch < wbytes) return bad_arg(c);
    if (!wbytes || !rows) return SVT_HIP_OK;
    return copy_2d(c, d, dpitch, h, hpitch, wbytes, rows, hipMemcpyHostToDevice, true);
}
int svt_hip_memcpy2d_d2h(SvtHipCtx* c, void* h, size_t hpitch, const void* d, size_t dpitch, size_t wbytes, size_t rows) {
    SVT_HIP_ENTER(c);
    if (!c || !d || !h || dpitch < wbytes || hpitch < wbytes) return bad_arg(c);
    if (!wbytes || !rows) return SVT_HIP_OK;
    return copy_2d(c, h, hpitch, d, dpitch, wbytes, rows, hipMemcpyDeviceToHost, true);
}
int svt_hip_memcpy2d_h2d_async(SvtHipCtx* c, void* d, size_t dpitch, const void* h, size_t hpitch, size_t wbytes, size_t rows) {
    SVT_HIP_ENTER(c);
    if (!c || !d || !h || dpitch < wbytes || hpitch < wbytes) return bad_arg(c);
    if (!wbytes || !rows) return SVT_HIP_OK;
    return copy_2d(c, d, dpitch, h, hpitch, wbytes, rows, hipMemcpyHostToDevice, false);
}
int svt_hip_memcpy2d_d2h_async(SvtHipCtx* c, void* h, size_t hpitch, const void* d, size_t dpitch, size_t wbytes, size_t rows) {
    SVT_HIP_ENTER(c);
    if (!c || !d || !h || dpitch < wbytes || hpitch < wbytes) return bad_arg(c);
    if (!wbytes || !rows) return SVT_HIP_OK;
    return copy_2d(c, h, hpitch, d, dpitch, wbytes, rows, hipMemcpyDeviceToHost, false);
}
int svt_hip_memcpy_h2d_async(SvtHipCtx* c, void* d, const void* h, size_t bytes) {
    SVT_HIP_ENTER(c);
    if (!c || (bytes && (!d || !h))) return bad_arg(c);
    if (!bytes) return SVT_HIP_OK;
    return copy_1d(c, d, h, bytes, hipMemcpyHostToDevice, false);
}
int svt_hip_memcpy_d2h_async(SvtHipCtx* c, void* h, const void* d, size_t bytes) {
    SVT_HIP_ENTER(c);
    if (!c || (bytes && (!d || !h))) return bad_arg(c);
    if (!bytes) return SVT_HIP_OK;
    return copy_1d(c, h, d, bytes, hipMemcpyDeviceToHost, false);
}
int svt_hip_device_count(int* count) {
    if (!count) return SVT_HIP_ERR_BAD_ARG;
    *count = 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 0) return SVT_HIP_ERR_NO_DEVICE;
    *count = n;
    return SVT_HIP_OK;
}
// Page-locks a buffer of the caller in place (the reference's picture buffers are allocated once per encoder instance): copies to and from it are then direct
// DMA at the link's rate instead of going through the runtime's pageable staging.
int svt_hip_host_register(SvtHipCtx* c, void* host, size_t bytes) {
    SVT_HIP_ENTER(c);
    if (!c || !host || !bytes) return bad_arg(c);
    const hipError_t e = hipHostRegister(host, bytes, hipHostRegisterDefault);
    if (e == hipErrorHostMemoryAlreadyRegistered) { (void)hipGetLastError(); return SVT_HIP_OK; }
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(c, e, "hipHostRegister"); }
    return SVT_HIP_OK;
}
int svt_hip_host_unregister(SvtHipCtx* c, void* host) {
    SVT_HIP_ENTER(c);
    if (!c || !host) return bad_arg(c);
    const hipError_t e = hipHostUnregister(host);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(c, e, "hipHostUnregister"); }
    return SVT_HIP_OK;
}
int svt_hip_host_alloc(SvtHipCtx* c, void** host, size_t bytes) {
    SVT_HIP_ENTER(c);
    if (!c || !host) return bad_arg(c);
    HIPCHK(c, hipHostMalloc(host, bytes ? bytes : 4, hipHostMallocDefault));
    return SVT_HIP_OK;
}
int svt_hip_host_free(SvtHipCtx* c, void* host) {
    SVT_HIP_ENTER(c);
    if (!c) return bad_arg(c);
    if (host) HIPCHK(c, hipHostFree(host));
    return SVT_HIP_OK;
}
#define SVT_HIP_TUS(X) X(cdef) X(cdef_select) X(comp_search) X(compound) X(conv) X(deblock) X(distortion) X(format) X(gm) X(gm_fit) X(gm_front) X(ibc_hash) X(ibc_search) X(ifs_search) X(intra) X(intra_cfl) X(md_pre) X(me_fullpel) X(obmc_search) X(palette) X(percall) X(pyramid) X(resize) X(scaled_pred) X(sgr) X(sgr_walk) X(tf_subpel) \
    X(tfilter) X(tpl) X(tpl_synth) X(txfm2d) X(warp) X(wiener)
#define X(n) int svt_hip_tu_probe_##n();
SVT_HIP_TUS(X)
#undef X
int svt_hip_warmup(SvtHipCtx* c) {
    SVT_HIP_ENTER(c);
    if (!c) return bad_arg(c);
    int bad = 0;
#define X(n) bad |= svt_hip_tu_probe_##n();
    SVT_HIP_TUS(X)
#undef X
    if (bad) { c->err = "svt_hip_warmup: a translation unit's code object did not load"; (void)hipGetLastError(); return SVT_HIP_ERR_RUNTIME; }
    return SVT_HIP_OK;
}
int svt_hip_timer_start(SvtHipCtx* c) {
    SVT_HIP_ENTER(c);
    if (!c) return bad_arg(c);
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    return SVT_HIP_OK;
}
int svt_hip_timer_stop_ms(SvtHipCtx* c, float* ms) {
    SVT_HIP_ENTER(c);
    if (!c || !ms) return bad_arg(c);
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    HIPCHK(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return SVT_HIP_OK;
}

/* ---------------------------------------------------------------------------------------- intra */
int svt_hip_intra_predict_batch_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_edges, const SvtHipIntraJob* d_jobs, int njobs, void* d_dst,
                                    int dst_stride) {
    SVT_HIP_ENTER(c);
    if (!c || !d_edges || !d_jobs || !d_dst || njobs < 0 || !fmt_ok(pix_bytes, bd) || dst_stride <= 0) return bad_arg(c, "svt_hip_intra_predict_batch_dev: bad argument");
    if (!njobs) return SVT_HIP_OK;
    return launched(c, svt_hip_launch_intra_predict(c->stream, pix_bytes, bd, d_edges, d_jobs, njobs, d_dst, dst_stride), "intra predict launch");
}

int svt_hip_intra_ois_picture_dev(SvtHipCtx* c, const uint8_t* d_src, int stride, int w, int h, int mode_end, uint8_t* d_mode, int32_t* d_cost) {
    SVT_HIP_ENTER(c);
    if (!c || !d_src || !d_mode || !d_cost || w < 16 || h < 16 || (w & 7) || (h & 7) || w > 65536 || h > 65536 || stride < ((w + 15) & ~15) || mode_end < 0 ||
        mode_end > 12)
        return bad_arg(c, "svt_hip_intra_ois_picture_dev: bad argument (w, h multiples of 8 and >= 16, stride >= ceil16(w), mode_end 0..12)");
    return launched(c, svt_hip_launch_intra_ois(c->stream, d_src, stride, w, h, mode_end, d_mode, d_cost), "intra ois launch");
}

int svt_hip_cfl_predict_batch_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_luma, int luma_stride, const void* d_edges, const SvtHipCflJob* d_jobs, int njobs,
                                  void* d_cb, void* d_cr, int chroma_stride, int16_t* d_ac) {
    SVT_HIP_ENTER(c);
    if (!c || !d_luma || !d_edges || !d_jobs || (!d_cb && !d_cr) || njobs < 0 || !fmt_ok(pix_bytes, bd) || luma_stride <= 0 || chroma_stride <= 0)
        return bad_arg(c, "svt_hip_cfl_predict_batch_dev: bad argument");
    if (!njobs) return SVT_HIP_OK;
    return launched(c, svt_hip_launch_cfl_predict(c->stream, pix_bytes, bd, d_luma, luma_stride, d_edges, d_jobs, njobs, d_cb, d_cr, chroma_stride, d_ac), "cfl predict launch");
}

int svt_hip_filter_intra_predict_batch_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_edges, const SvtHipFilterIntraJob* d_jobs, int njobs, void* d_dst,
                                           int dst_stride) {
    SVT_HIP_ENTER(c);
    if (!c || !d_edges || !d_jobs || !d_dst || njobs < 0 || !fmt_ok(pix_bytes, bd) || dst_stride <= 0)
        return bad_arg(c, "svt_hip_filter_intra_predict_batch_dev: bad argument");
    if (!njobs) return SVT_HIP_OK;
    return launched(c, svt_hip_launch_filter_intra_predict(c->stream, pix_bytes, bd, d_edges, d_jobs, njobs, d_dst, dst_stride), "filter-intra predict launch");
}

/* ---------------------------------------------------------------------------------- palette luma search, screen-content detection (palette.hip) */
int svt_hip_palette_search_batch_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_plane, int stride, const SvtHipPaletteJob* d_jobs, int njobs,
                                     SvtHipPaletteResult* d_results, SvtHipPaletteCand* d_cands, uint8_t* d_maps) {
    SVT_HIP_ENTER(c);
    if (!c || !d_plane || !d_jobs || !d_results || !d_cands || !d_maps || njobs < 0 || !fmt_ok(pix_bytes, bd) || stride <= 0)
        return bad_arg(c, "svt_hip_palette_search_batch_dev: bad argument");
    if (!njobs) return SVT_HIP_OK;
    return launched(c, svt_hip_launch_palette_search(c->stream, pix_bytes, bd, d_plane, stride, d_jobs, njobs, d_results, d_cands, d_maps), "palette search launch");
}

int svt_hip_screen_content_detect_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_plane, int stride, int width, int height, int32_t* d_out) {
    SVT_HIP_ENTER(c);
    if (!c || !d_plane || !d_out || !((pix_bytes == 1 && bd == 8) || (pix_bytes == 2 && bd == 10)) || stride <= 0 || width < 1 || height < 1 ||
        (int64_t)width * height > INT32_MAX)
        return bad_arg(c, "svt_hip_screen_content_detect_dev: bad argument (pix_bytes 1 with bd 8 or pix_bytes 2 with bd 10, stride > 0, width and height >= 1)");
    return launched(c, svt_hip_launch_screen_content_detect(c->stream, pix_bytes, d_plane, stride, width, height, d_out), "screen-content detect launch");
}

/* ---------------------------------------------------------------------------------- intra block copy: hash planes, hash table, hash search (ibc_hash.hip) */
size_t svt_hip_ibc_hash_scratch_bytes(int width, int height) { return ibc::picture_ok(width, width, height) ? ibc::scratch_layout(width, height).total : 0; }
size_t svt_hip_ibc_hash_max_entries(int width, int height) { return ibc::picture_ok(width, width, height) ? (size_t)ibc::max_entries(width, height) : 0; }
static bool ibc_scratch_ok(const void* d_scratch, size_t scratch_bytes, int width, int height) {
    return d_scratch && !((uintptr_t)d_scratch & 255) && scratch_bytes >= ibc::scratch_layout(width, height).total;
}

int svt_hip_ibc_block_hashes_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_luma, int stride, int width, int height, int block_size, uint32_t* d_hash1,
                                 uint32_t* d_hash2, int8_t* d_same, void* d_scratch, size_t scratch_bytes) {
    SVT_HIP_ENTER(c);
    if (!c || !d_luma || !d_hash1 || !d_hash2 || !d_same || !ibc::fmt_ok(pix_bytes, bd) || !ibc::picture_ok(stride, width, height) ||
        (block_size != 2 && ibc::size_index(block_size) < 0) || !ibc_scratch_ok(d_scratch, scratch_bytes, width, height))
        return bad_arg(c, "svt_hip_ibc_block_hashes_dev: bad argument");
    return launched(c, svt_hip_launch_ibc_block_hashes(c->stream, pix_bytes, d_luma, stride, width, height, block_size, d_hash1, d_hash2, d_same, d_scratch),
                    "intra-block-copy block hashes launch");
}

int svt_hip_ibc_hash_table_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_luma, int stride, int width, int height, int32_t* d_bucket_start,
                               SvtHipIbcHashEntry* d_entries, int64_t capacity, int32_t* d_info, void* d_scratch, size_t scratch_bytes) {
    SVT_HIP_ENTER(c);
    if (!c || !d_luma || !d_bucket_start || !d_info || (!d_entries && capacity) || capacity < 0 || !ibc::fmt_ok(pix_bytes, bd) || !ibc::picture_ok(stride, width, height) ||
        !ibc_scratch_ok(d_scratch, scratch_bytes, width, height))
        return bad_arg(c, "svt_hip_ibc_hash_table_dev: bad argument");
    return launched(c, svt_hip_launch_ibc_hash_table(c->stream, pix_bytes, d_luma, stride, width, height, d_bucket_start, d_entries, capacity, d_info, d_scratch),
                    "intra-block-copy hash table launch");
}

int svt_hip_ibc_hash_search_batch_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_luma, int stride, int width, int height, const int32_t* d_bucket_start,
                                      const SvtHipIbcHashEntry* d_entries, const int32_t* d_mv_joint_cost, const int32_t* d_mv_comp_cost, const SvtHipIbcSearchJob* d_jobs,
                                      int njobs, SvtHipIbcSearchResult* d_results) {
    SVT_HIP_ENTER(c);
    if (!c || !ibc::search_args_ok(pix_bytes, bd, d_luma, stride, width, height, d_bucket_start, d_entries, d_mv_joint_cost, d_mv_comp_cost, d_jobs, njobs, d_results))
        return bad_arg(c, "svt_hip_ibc_hash_search_batch_dev: bad argument");
    if (!njobs) return SVT_HIP_OK;
    return launched(c, svt_hip_launch_ibc_hash_search(c->stream, pix_bytes, bd, d_luma, stride, width, height, d_bucket_start, d_entries, d_mv_joint_cost, d_mv_comp_cost,
                                                      d_jobs, njobs, d_results),
                    "intra-block-copy hash search launch");
}

/* ---------------------------------------------------------------------------------- intra block copy: diamond, mesh and the final choice (ibc_search.hip) */
size_t svt_hip_ibc_full_search_scratch_bytes(int njobs) { return njobs < 0 ? 0 : ibcs::full_scratch(njobs).total; }

int svt_hip_ibc_full_search_batch_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_luma, int stride, int width, int height, const int32_t* d_bucket_start,
                                      const SvtHipIbcHashEntry* d_entries, const int32_t* d_mv_joint_cost, const int32_t* d_mv_comp_cost, const int32_t* mesh_patterns,
                                      const SvtHipIbcFullSearchJob* d_jobs, int njobs, SvtHipIbcFullSearchResult* d_results, void* d_scratch, size_t scratch_bytes) {
    SVT_HIP_ENTER(c);
    if (!c || !d_luma || !d_mv_joint_cost || !d_mv_comp_cost || !d_jobs || !d_results || njobs < 0 || njobs > ibcs::MAX_JOBS || !ibc::fmt_ok(pix_bytes, bd) ||
        !ibc::picture_ok(stride, width, height))
        return bad_arg(c, "svt_hip_ibc_full_search_batch_dev: bad argument");
    if (!d_bucket_start != !d_entries) return bad_arg(c, "svt_hip_ibc_full_search_batch_dev: bad argument (the two table pointers are both given or both NULL)");
    if (!ibcs::patterns_ok(mesh_patterns))
        return bad_arg(c, "svt_hip_ibc_full_search_batch_dev: bad argument (a mesh pattern the walk can reach has interval < 1 or range outside 1 .. 256)");
    if (!d_scratch || ((uintptr_t)d_scratch & 255) || scratch_bytes < ibcs::full_scratch(njobs).total)
        return bad_arg(c, "svt_hip_ibc_full_search_batch_dev: bad argument (d_scratch: svt_hip_ibc_full_search_scratch_bytes(njobs), 256-byte aligned)");
    if (!njobs) return SVT_HIP_OK;
    return launched(c, svt_hip_launch_ibc_full_search(c->stream, pix_bytes, bd, d_luma, stride, width, height, d_bucket_start, d_entries, d_mv_joint_cost, d_mv_comp_cost,
                                                      mesh_patterns, d_jobs, njobs, d_results, d_scratch),
                    "intra-block-copy full search launch");
}

/* ---------------------------------------------------------------------------------- masked compound and inter-intra: choosing the mask (comp_search.hip) */
size_t svt_hip_wedge_mask_table_bytes(void) { return cs::WEDGE_TABLE_BYTES; }
int    svt_hip_wedge_mask_offset(int bsize, int sign, int index) { return cs::wedge_offset(bsize, sign, index); }

static int wedge_masks(SvtHipCtx* c) {
    if (c->wedge_masks) return SVT_HIP_OK;
    std::vector<uint8_t> table(cs::WEDGE_TABLE_BYTES);
    cs::wedge_table_build(table.data());
    HIPCHK(c, hipMalloc((void**)&c->wedge_masks, table.size()));
    hipError_t e = hipMemcpy(c->wedge_masks, table.data(), table.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(c->wedge_masks); c->wedge_masks = nullptr; return fail(c, e, "wedge mask table upload"); }
    return SVT_HIP_OK;
}

int svt_hip_wedge_masks_dev(SvtHipCtx* c, const uint8_t** d_masks) {
    SVT_HIP_ENTER(c);
    if (!c || !d_masks) return bad_arg(c, "svt_hip_wedge_masks_dev: bad argument");
    if (int rc = wedge_masks(c)) return rc;
    *d_masks = c->wedge_masks;
    return SVT_HIP_OK;
}

namespace {
constexpr size_t kRdGridDoubles = (size_t)(cs::RATE_CATS + cs::DIST_CATS) * cs::GRID_COLS, kRdGridBytes = kRdGridDoubles * sizeof(double) + cs::BLOCK_SIZES * sizeof(int32_t);
}
int svt_hip_set_rd_curvfit_grids(SvtHipCtx* c, const double* rate, const double* dist, const int32_t* bsize_cat) {
    SVT_HIP_ENTER(c);
    if (!c || !cs::rd_tables_ok(rate, dist, bsize_cat)) return bad_arg(c, "svt_hip_set_rd_curvfit_grids: bad argument (three tables, every category 0 .. 3)");
    uint8_t host[kRdGridBytes];
    memcpy(host, rate, (size_t)cs::RATE_CATS * cs::GRID_COLS * sizeof(double));
    memcpy(host + (size_t)cs::RATE_CATS * cs::GRID_COLS * sizeof(double), dist, (size_t)cs::DIST_CATS * cs::GRID_COLS * sizeof(double));
    memcpy(host + kRdGridDoubles * sizeof(double), bsize_cat, cs::BLOCK_SIZES * sizeof(int32_t));
    if (!c->rd_grids) HIPCHK(c, hipMalloc(&c->rd_grids, kRdGridBytes));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // a search still in flight reads the tables it was launched with
    HIPCHK(c, hipMemcpy(c->rd_grids, host, kRdGridBytes, hipMemcpyHostToDevice));
    c->rd_grids_set = true;
    return SVT_HIP_OK;
}

int svt_hip_compound_search_batch_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_src, int src_stride, int width, int height, const void* d_pred,
                                      int64_t pred_samples, const int32_t* d_rates, int nrates, const SvtHipCompSearchJob* jobs, int njobs,
                                      SvtHipCompSearchResult* d_results, SvtHipCompSearchCand* d_cand) {
    SVT_HIP_ENTER(c);
    if (!c || !cs::search_args_ok(pix_bytes, bd, d_src, src_stride, width, height, d_pred, pred_samples, d_rates, nrates, jobs, njobs, d_results))
        return bad_arg(c, "svt_hip_compound_search_batch_dev: bad argument");
    if (!c->rd_grids_set) return bad_arg(c, "svt_hip_compound_search_batch_dev: bad argument (svt_hip_set_rd_curvfit_grids has not been called on this context)");
    if (!njobs) return SVT_HIP_OK;
    if (int rc = wedge_masks(c)) return rc;
    const size_t bytes = (size_t)njobs * sizeof(SvtHipCompSearchJob);
    if (bytes > c->comp_jobs_bytes) {
        HIPCHK(c, hipStreamSynchronize(c->stream));   // an earlier search may still read the old list
        if (c->comp_jobs) (void)hipFree(c->comp_jobs);
        c->comp_jobs = nullptr;
        c->comp_jobs_bytes = 0;
        HIPCHK(c, hipMalloc(&c->comp_jobs, bytes));
        c->comp_jobs_bytes = bytes;
    }
    HIPCHK(c, hipMemcpyAsync(c->comp_jobs, jobs, bytes, hipMemcpyHostToDevice, c->stream));
    const double* grids = (const double*)c->rd_grids;
    return launched(c, svt_hip_launch_compound_search(c->stream, pix_bytes, bd, d_src, src_stride, d_pred, d_rates, c->wedge_masks, grids,
                                                      grids + (size_t)cs::RATE_CATS * cs::GRID_COLS, (const int32_t*)(grids + kRdGridDoubles),
                                                      (const SvtHipCompSearchJob*)c->comp_jobs, njobs, d_results, d_cand),
                    "compound search launch");
}

/* ---------------------------------------------------------------------------------- OBMC in mode decision: weighted target and motion refinement (obmc_search.hip) */
// svt_hip_obmc_target_batch_dev: calc_target_weighted_pred (Encoder/Codec/EbEncInterPrediction.c:2376-2437) with its visitors (:2196-2256) for a list of blocks.
// svt_hip_obmc_search_batch_dev: single_motion_search (Encoder/Codec/EbModeDecision.c:2951-3036) = svt_av1_obmc_full_pixel_search (Encoder/Codec/av1me.c:836-855) +
// svt_av1_find_best_obmc_sub_pixel_tree_up (:1069-1254) + svt_av1_mv_bit_cost.  What each refuses is obmc::target_args_ok / obmc::search_args_ok, shared with the host forms.
// the job list of a call, host memory that has been checked, in the context's staging buffer `slot`: stream-ordered, grown on demand
static int stage_jobs(SvtHipCtx* c, int slot, const void* jobs, size_t bytes) {
    if (bytes > c->job_stage_bytes[slot]) {
        HIPCHK(c, hipStreamSynchronize(c->stream));   // an earlier call may still read the old list
        if (c->job_stage[slot]) (void)hipFree(c->job_stage[slot]);
        c->job_stage[slot] = nullptr;
        c->job_stage_bytes[slot] = 0;
        HIPCHK(c, hipMalloc(&c->job_stage[slot], bytes));
        c->job_stage_bytes[slot] = bytes;
    }
    HIPCHK(c, hipMemcpyAsync(c->job_stage[slot], jobs, bytes, hipMemcpyHostToDevice, c->stream));
    return SVT_HIP_OK;
}

int svt_hip_obmc_target_batch_dev(SvtHipCtx* c, const uint8_t* d_src, int src_stride, int width, int height, const uint8_t* d_nbr, int64_t nbr_samples,
                                  const SvtHipObmcTargetJob* jobs, int njobs, int32_t* d_wsrc, int32_t* d_mask, int64_t wm_samples) {
    SVT_HIP_ENTER(c);
    if (!c || !obmc::target_args_ok(d_src, src_stride, width, height, d_nbr, nbr_samples, jobs, njobs, d_wsrc, d_mask, wm_samples))
        return bad_arg(c, "svt_hip_obmc_target_batch_dev: bad argument");
    if (!njobs) return SVT_HIP_OK;
    if (int rc = stage_jobs(c, 0, jobs, (size_t)njobs * sizeof(SvtHipObmcTargetJob))) return rc;
    return launched(c, svt_hip_launch_obmc_target(c->stream, d_src, src_stride, d_nbr, (const SvtHipObmcTargetJob*)c->job_stage[0], njobs, d_wsrc, d_mask),
                    "OBMC target launch");
}

int svt_hip_obmc_search_batch_dev(SvtHipCtx* c, const uint8_t* d_ref, int ref_stride, int width, int height, int pad_w, int pad_h, int mi_rows, int mi_cols,
                                  const int32_t* d_wsrc, const int32_t* d_mask, int64_t wm_samples, const int32_t* d_mv_joint_cost, const int32_t* d_mv_comp_cost,
                                  const SvtHipObmcSearchJob* jobs, int njobs, SvtHipObmcSearchResult* d_results) {
    SVT_HIP_ENTER(c);
    const obmc::Plane P{d_ref, ref_stride, width, height, pad_w, pad_h, mi_rows, mi_cols};
    if (!c || !obmc::search_args_ok(P, d_wsrc, d_mask, wm_samples, d_mv_joint_cost, d_mv_comp_cost, jobs, njobs, d_results))
        return bad_arg(c, "svt_hip_obmc_search_batch_dev: bad argument");
    if (!njobs) return SVT_HIP_OK;
    if (int rc = stage_jobs(c, 1, jobs, (size_t)njobs * sizeof(SvtHipObmcSearchJob))) return rc;
    return launched(c, svt_hip_launch_obmc_search(c->stream, d_ref, ref_stride, width, height, pad_w, pad_h, mi_rows, mi_cols, d_wsrc, d_mask, wm_samples, d_mv_joint_cost,
                                                  d_mv_comp_cost, (const SvtHipObmcSearchJob*)c->job_stage[1], njobs, d_results),
                    "OBMC search launch");
}

/* ---------------------------------------------------------------------------------- the dual interpolation filter search of mode decision (ifs_search.hip) */
// interpolation_filter_search (Encoder/Codec/EbEncInterPrediction.c:3047-3297) for a list of blocks.  What it refuses is ifs::search_args_ok, shared with the host form.
int svt_hip_ifs_search_batch_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_src, int src_stride, int width, int height, const void* d_ref0, int ref0_stride,
                                 const void* d_ref1, int ref1_stride, void* d_dst, int dst_stride, const SvtHipIfsJob* jobs, int njobs, SvtHipIfsResult* d_results,
                                 SvtHipIfsCand* d_cand) {
    SVT_HIP_ENTER(c);
    if (!c || !ifs::search_args_ok(pix_bytes, bd, d_src, src_stride, width, height, d_ref0, ref0_stride, d_ref1, ref1_stride, d_dst, dst_stride, jobs, njobs, d_results))
        return bad_arg(c, "svt_hip_ifs_search_batch_dev: bad argument");
    if (!njobs) return SVT_HIP_OK;
    if (int rc = stage_jobs(c, 2, jobs, (size_t)njobs * sizeof(SvtHipIfsJob))) return rc;
    return launched(c, svt_hip_launch_ifs_search(c->stream, pix_bytes, bd, d_src, src_stride, d_ref0, ref0_stride, d_ref1, ref1_stride, d_dst, dst_stride,
                                                 (const SvtHipIfsJob*)c->job_stage[2], njobs, d_results, d_cand),
                    "interpolation filter search launch");
}

/* ---------------------------------------------------------------------------------- TPL dispenser */
/* one decision byte per macroblock (phase A -> the step launches), rounded up to a cache line */
size_t svt_hip_tpl_dispenser_scratch_bytes(int w, int h) {
    if (w <= 0 || h <= 0) return 256;
    return (((size_t)((w + 15) / 16) * (size_t)((h + 15) / 16) + 255) & ~(size_t)255) + 256;
}

int svt_hip_tpl_dispenser_picture_dev(SvtHipCtx* c, const SvtHipTplParams* p, const uint8_t* d_cur, int cur_stride, const SvtHipTplRef refs[7],
                                      const uint32_t* d_mv, const uint8_t* d_ref_mask, const uint8_t* d_ois_mode, const int32_t* d_ois_cost, uint8_t* d_recon,
                                      int recon_stride, SvtHipTplMbStats* d_stats, void* d_scratch) {
    SVT_HIP_ENTER(c);
    bool bad = !c || !p || !d_cur || !refs || !d_recon || !d_stats || !d_scratch;
    if (!bad) {
        const int w16 = (p->w + 15) & ~15;
        bad = p->w < 16 || p->h < 16 || (p->w & 7) || (p->h & 7) || p->w > 65536 || p->h > 65536 || p->pad < 16 || p->pad > 65536 || cur_stride < w16 ||
              recon_stride < w16 || p->q.variant != 2 || p->q.log_scale != 0 || (p->use_ois && (!d_ois_mode || !d_ois_cost));
        for (int r = 0; r < 7 && !bad; r++)
            if (refs[r].d_src) bad = !refs[r].d_rec || refs[r].d_rec == d_recon || refs[r].src_stride < w16 || refs[r].rec_stride < w16 || !d_mv || !d_ref_mask;
    }
    if (bad) return bad_arg(c, "svt_hip_tpl_dispenser_picture_dev: bad argument (w, h multiples of 8 and >= 16, strides >= ceil16(w), pad >= 16, q.variant 2, q.log_scale 0)");
    if (int rc = launched(c, svt_hip_launch_tpl_dispenser(c->stream, p, d_cur, cur_stride, refs, d_mv, d_ref_mask, d_ois_mode, d_ois_cost, d_recon, recon_stride, d_stats,
                                                          (uint8_t*)d_scratch, c->tpl_phases), "tpl dispenser launch"))
        return rc;
    if (!(c->tpl_phases & 4)) return SVT_HIP_OK;
    return launched(c, svt_hip_launch_generate_padding(c->stream, d_recon, 1, recon_stride, p->w, p->h, p->pad, p->pad), "tpl dispenser padding launch");
}

int svt_hip_tpl_set_phases(SvtHipCtx* c, int mask) {
    if (!c || mask < 0 || mask > 7) return bad_arg(c);
    c->tpl_phases = mask;
    return SVT_HIP_OK;
}

/* ---------------------------------------------------------------------------------- TPL synthesizer, r0 / beta */
size_t svt_hip_tpl_dep_bytes(int w, int h, int cell_log2) {
    if (!tplsyn::size_ok(w, h) || (cell_log2 != 3 && cell_log2 != 4)) return 0;
    return tplsyn::dep_cells(tplsyn::geom(w, h, cell_log2)) * 2 * sizeof(int64_t);
}
size_t svt_hip_tpl_r0beta_out_bytes(int w, int h, int sb_size) {
    if (!tplsyn::size_ok(w, h) || (sb_size != 64 && sb_size != 128)) return 0;
    return tplsyn::out_bytes(w, h, sb_size);
}
size_t svt_hip_tpl_r0beta_scratch_bytes(void) { return 256; }   // the two base sums, a cache line of their own

// what the entry points refuse alike, as one test (docs/design/kernels-overview.md); the texts stay literals at the call sites
enum { TPL_SYNTH_FINE = 0, TPL_SYNTH_RATE, TPL_SYNTH_PARAMS, TPL_SYNTH_SELF, TPL_SYNTH_FRAMES };
static int tpl_synth_refusal(const SvtHipTplSynthParams* p, const SvtHipTplWindowFrame* frames, int n_frames, bool with_frames) {
    if (p && p->rate != 0) return TPL_SYNTH_RATE;
    if (!tplsyn::params_ok(p)) return TPL_SYNTH_PARAMS;
    const int bad = with_frames ? tplsyn::frames_check(frames, n_frames) : 0;
    return bad == 2 ? TPL_SYNTH_SELF : bad ? TPL_SYNTH_FRAMES : TPL_SYNTH_FINE;
}

static int tpl_synth_launch(SvtHipCtx* c, const SvtHipTplSynthParams* p, const SvtHipTplWindowFrame* frames, int idx) {
    const SvtHipTplWindowFrame& f = frames[idx];
    int64_t* target[8];
    for (int k = 0; k < 8; k++) target[k] = f.ref_window[k] < 0 ? nullptr : frames[f.ref_window[k]].d_dep;
    return launched(c, svt_hip_launch_tpl_synth(c->stream, p->w, p->h, p->cell_log2, f.d_stats, f.d_dep, target), "tpl synthesizer launch");
}

int svt_hip_tpl_synth_picture_dev(SvtHipCtx* c, const SvtHipTplSynthParams* p, const SvtHipTplWindowFrame* frames, int n_frames, int frame_idx) {
    SVT_HIP_ENTER(c);
    if (!c) return bad_arg(c);
    switch (tpl_synth_refusal(p, frames, n_frames, true)) {
    case TPL_SYNTH_RATE: return bad_arg(c, "svt_hip_tpl_synth_picture_dev: rate must be 0 (the reference's tpl_opt_flag == 1; delta_rate_cost is not built)");
    case TPL_SYNTH_PARAMS: return bad_arg(c, "svt_hip_tpl_synth_picture_dev: bad argument (w, h multiples of 8 and >= 16, cell_log2 3 or 4, sb_size 64 or 128, base_rdmult >= 0)");
    case TPL_SYNTH_SELF: return bad_arg(c, "svt_hip_tpl_synth_picture_dev: ref_window[1..7] names the picture itself (the result would depend on the order of the blocks)");
    case TPL_SYNTH_FRAMES:
        return bad_arg(c, "svt_hip_tpl_synth_picture_dev: bad argument (1 <= n_frames <= 60, every d_dep distinct and non-NULL, d_stats of picture 0 and of every picture "
                          "that is on, -1 <= ref_window[k] < n_frames)");
    }
    if (frame_idx < 0 || frame_idx >= n_frames) return bad_arg(c, "svt_hip_tpl_synth_picture_dev: bad argument (0 <= frame_idx < n_frames)");
    if (!frames[frame_idx].on) return SVT_HIP_OK;
    return tpl_synth_launch(c, p, frames, frame_idx);
}

int svt_hip_tpl_r0beta_dev(SvtHipCtx* c, const SvtHipTplSynthParams* p, const SvtHipTplMbStats* d_stats, const int64_t* d_dep, void* d_out, void* d_scratch) {
    SVT_HIP_ENTER(c);
    if (!c) return bad_arg(c);
    switch (tpl_synth_refusal(p, nullptr, 0, false)) {
    case TPL_SYNTH_RATE: return bad_arg(c, "svt_hip_tpl_r0beta_dev: rate must be 0 (the reference's tpl_opt_flag == 1; delta_rate_cost is not built)");
    case TPL_SYNTH_PARAMS: return bad_arg(c, "svt_hip_tpl_r0beta_dev: bad argument (w, h multiples of 8 and >= 16, cell_log2 3 or 4, sb_size 64 or 128, base_rdmult >= 0)");
    }
    if (!d_stats || !d_dep || !d_out || !d_scratch || ((uintptr_t)d_out & 7) || ((uintptr_t)d_scratch & 7))
        return bad_arg(c, "svt_hip_tpl_r0beta_dev: bad argument (d_stats, d_dep, d_out, d_scratch non-NULL, d_out and d_scratch 8-byte aligned)");
    return launched(c, svt_hip_launch_tpl_r0beta(c->stream, p, d_stats, d_dep, d_out, d_scratch), "tpl r0/beta launch");
}

int svt_hip_tpl_window_dev(SvtHipCtx* c, const SvtHipTplSynthParams* p, const SvtHipTplWindowFrame* frames, int n_frames, void* d_out, void* d_scratch) {
    SVT_HIP_ENTER(c);
    if (!c) return bad_arg(c);
    switch (tpl_synth_refusal(p, frames, n_frames, true)) {
    case TPL_SYNTH_RATE: return bad_arg(c, "svt_hip_tpl_window_dev: rate must be 0 (the reference's tpl_opt_flag == 1; delta_rate_cost is not built)");
    case TPL_SYNTH_PARAMS: return bad_arg(c, "svt_hip_tpl_window_dev: bad argument (w, h multiples of 8 and >= 16, cell_log2 3 or 4, sb_size 64 or 128, base_rdmult >= 0)");
    case TPL_SYNTH_SELF: return bad_arg(c, "svt_hip_tpl_window_dev: ref_window[1..7] names the picture itself (the result would depend on the order of the blocks)");
    case TPL_SYNTH_FRAMES:
        return bad_arg(c, "svt_hip_tpl_window_dev: bad argument (1 <= n_frames <= 60, every d_dep distinct and non-NULL, d_stats of picture 0 and of every picture that is "
                          "on, -1 <= ref_window[k] < n_frames)");
    }
    if (!d_out || !d_scratch || ((uintptr_t)d_out & 7) || ((uintptr_t)d_scratch & 7))
        return bad_arg(c, "svt_hip_tpl_window_dev: bad argument (d_out, d_scratch non-NULL and 8-byte aligned)");
    const size_t bytes = svt_hip_tpl_dep_bytes(p->w, p->h, p->cell_log2);
    for (int i = 0; i < n_frames; i++) HIPCHK(c, hipMemsetAsync(frames[i].d_dep, 0, bytes, c->stream));   // :1159-1163
    for (int i = n_frames - 1; i >= 0; i--)                                                                // :1181-1194
        if (frames[i].on)
            if (int rc = tpl_synth_launch(c, p, frames, i)) return rc;
    return launched(c, svt_hip_launch_tpl_r0beta(c->stream, p, frames[0].d_stats, frames[0].d_dep, d_out, d_scratch), "tpl r0/beta launch");   // :1197
}

/* ---------------------------------------------------------------------------------- global motion */
int svt_hip_gm_error_table(uint16_t out[512]) {
    if (!out) return SVT_HIP_ERR_BAD_ARG;
    std::memcpy(out, svt_hip_gm_error_lut_host(), 512 * sizeof(uint16_t));
    return SVT_HIP_OK;
}

static int gm_lut(SvtHipCtx* c) {
    if (c->gm_lut) return SVT_HIP_OK;
    HIPCHK(c, hipMalloc((void**)&c->gm_lut, 512 * sizeof(uint16_t)));
    hipError_t e = hipMemcpy(c->gm_lut, svt_hip_gm_error_lut_host(), 512 * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(c->gm_lut); c->gm_lut = nullptr; return fail(c, e, "global-motion error table upload"); }
    return SVT_HIP_OK;
}

static bool gm_plane_bad(const uint8_t* p, int stride, int w, int h) {
    return !p || w < 8 || h < 8 || w > SVT_HIP_GM_MAX_DIM || h > SVT_HIP_GM_MAX_DIM || stride < w;
}

int svt_hip_gm_shear_params_batch_dev(SvtHipCtx* c, const int32_t* d_wmmat, int n, SvtHipGmModel* d_out) {
    SVT_HIP_ENTER(c);
    if (!c || n < 0 || n > SVT_HIP_GM_MAX_MODELS || !d_wmmat || !d_out) return bad_arg(c, "svt_hip_gm_shear_params_batch_dev: bad argument");
    return launched(c, svt_hip_launch_gm_shear_params(c->stream, d_wmmat, n, d_out), "global-motion shear parameter launch");
}

int svt_hip_gm_warp_error_batch_dev(SvtHipCtx* c, const uint8_t* d_src, int src_stride, int w, int h, const uint8_t* d_ref, int ref_width, int ref_height, int ref_stride,
                                    const SvtHipGmModel* d_models, int n, int64_t* d_err) {
    SVT_HIP_ENTER(c);
    if (!c || gm_plane_bad(d_src, src_stride, w, h) || gm_plane_bad(d_ref, ref_stride, ref_width, ref_height) || n < 0 || n > SVT_HIP_GM_MAX_MODELS || !d_models || !d_err)
        return bad_arg(c, "svt_hip_gm_warp_error_batch_dev: bad argument (planes 8 .. 16384 wide and high, stride >= width, 0 <= n <= 2^20)");
    if (!n) return SVT_HIP_OK;
    if (int rc = gm_lut(c)) return rc;
    const SvtHipGmRef r = {d_ref, ref_width, ref_height, ref_stride, 0};
    return launched(c, svt_hip_launch_gm_warp_error(c->stream, d_src, src_stride, w, h, &r, d_models, n, c->gm_lut, d_err), "global-motion warp error launch");
}

int svt_hip_gm_frame_error_batch_dev(SvtHipCtx* c, const uint8_t* d_src, int src_stride, int w, int h, const SvtHipGmRef* refs, int n_refs, int64_t* d_err) {
    SVT_HIP_ENTER(c);
    bool bad = !c || gm_plane_bad(d_src, src_stride, w, h) || n_refs < 0 || n_refs > SVT_HIP_GM_MAX_REFS || !refs || !d_err;
    for (int i = 0; i < n_refs && !bad; i++) bad = !refs[i].d_plane || refs[i].stride < w;
    if (bad) return bad_arg(c, "svt_hip_gm_frame_error_batch_dev: bad argument (0 <= n_refs <= 8, every plane's stride >= w)");
    if (!n_refs) return SVT_HIP_OK;
    if (int rc = gm_lut(c)) return rc;
    return launched(c, svt_hip_launch_gm_frame_error(c->stream, d_src, src_stride, w, h, refs, n_refs, c->gm_lut, d_err), "global-motion frame error launch");
}

size_t svt_hip_gm_refine_scratch_bytes(int njobs) { return svt_hip_gm_refine_scratch_layout_bytes(njobs); }

/* Rounds are enqueued in chunks and the done counter is read once per chunk.  The first chunk is what a walk needs when no directional run outlives the
 * speculation (the initial error + one round per parameter and refinement of a 5-refinement AFFINE walk); a round after every job has finished costs two
 * launches whose workgroups exit at once. */
int svt_hip_gm_refine_picture_dev(SvtHipCtx* c, const uint8_t* d_src, int src_stride, int w, int h, const SvtHipGmRef* refs, int n_refs, const SvtHipGmJob* d_jobs,
                                  int njobs, SvtHipGmResult* d_results, void* d_scratch, int* polls_out) {
    SVT_HIP_ENTER(c);
    bool bad = !c || gm_plane_bad(d_src, src_stride, w, h) || n_refs < 1 || n_refs > SVT_HIP_GM_MAX_REFS || !refs || njobs < 0 || njobs > SVT_HIP_GM_MAX_JOBS ||
               !d_jobs || !d_results || !d_scratch || ((uintptr_t)d_scratch & 7);
    for (int i = 0; i < n_refs && !bad; i++) bad = gm_plane_bad(refs[i].d_plane, refs[i].stride, refs[i].width, refs[i].height);
    if (bad) return bad_arg(c, "svt_hip_gm_refine_picture_dev: bad argument (planes 8 .. 16384 wide and high, stride >= width, 1 <= n_refs <= 8, 0 <= njobs <= 1024)");
    if (polls_out) *polls_out = 0;
    if (!njobs) return SVT_HIP_OK;
    if (int rc = gm_lut(c)) return rc;
    const int* d_done = svt_hip_gm_done_counter(d_scratch, njobs);
    int polls = 0;
    for (int chunk = 0;; chunk++) {
        const int rounds = chunk ? 8 : 32;
        if (int rc = launched(c, svt_hip_launch_gm_refine_rounds(c->stream, d_src, src_stride, w, h, refs, n_refs, d_jobs, njobs, d_results, d_scratch, c->gm_lut, chunk == 0, rounds),
                              "global-motion refinement launch"))
            return rc;
        int done = 0;
        HIPCHK(c, hipMemcpyAsync(&done, d_done, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        polls++;
        if (done >= njobs) break;
        if (chunk > (1 << 16)) { c->err = "svt_hip_gm_refine_picture_dev: the walk did not end"; return SVT_HIP_ERR_RUNTIME; }
    }
    if (polls_out) *polls_out = polls;
    return SVT_HIP_OK;
}

/* the front half: corners and correspondences (gm_front.hip) */
static bool gm_planes_bad(const SvtHipGmRef* p, int n) {
    bool bad = !p;
    for (int i = 0; i < n && !bad; i++) bad = gm_plane_bad(p[i].d_plane, p[i].stride, p[i].width, p[i].height);
    return bad;
}

size_t svt_hip_gm_corners_scratch_bytes(const SvtHipGmRef* planes, int n_planes) {
    if (n_planes < 1 || n_planes > 1 + SVT_HIP_GM_MAX_REFS || gm_planes_bad(planes, n_planes)) return 0;
    return svt_hip_gm_corners_scratch_layout_bytes(planes, n_planes);
}

int svt_hip_gm_corners_batch_dev(SvtHipCtx* c, const SvtHipGmRef* planes, int n_planes, int max_points, int32_t* d_points, int32_t* d_counts, int32_t* d_kept,
                                 void* d_scratch) {
    SVT_HIP_ENTER(c);
    if (!c || n_planes < 1 || n_planes > 1 + SVT_HIP_GM_MAX_REFS || gm_planes_bad(planes, n_planes) || max_points < 1 || max_points > SVT_HIP_GM_MAX_CORNERS || !d_points ||
        !d_counts || !d_scratch || ((uintptr_t)d_scratch & 7))
        return bad_arg(c, "svt_hip_gm_corners_batch_dev: bad argument (1 <= n_planes <= 9, planes 8 .. 16384 wide and high, stride >= width, 1 <= max_points <= 4096)");
    return launched(c, svt_hip_launch_gm_corners(c->stream, planes, n_planes, max_points, d_points, d_counts, d_kept, d_scratch), "global-motion corner launch");
}

int svt_hip_gm_cross_correlation_batch_dev(SvtHipCtx* c, const uint8_t* d_im1, int stride1, const uint8_t* d_im2, int stride2, int w, int h, const int32_t* d_pairs, int n,
                                           double* d_out) {
    SVT_HIP_ENTER(c);
    if (!c || gm_plane_bad(d_im1, stride1, w, h) || gm_plane_bad(d_im2, stride2, w, h) || n < 0 || n > SVT_HIP_GM_MAX_MODELS || !d_pairs || !d_out)
        return bad_arg(c, "svt_hip_gm_cross_correlation_batch_dev: bad argument (planes 8 .. 16384 wide and high, strides >= w, 0 <= n <= 2^20)");
    return launched(c, svt_hip_launch_gm_cross_correlation(c->stream, d_im1, stride1, d_im2, stride2, w, h, d_pairs, n, d_out), "global-motion cross-correlation launch");
}

int svt_hip_gm_correspondences_batch_dev(SvtHipCtx* c, const uint8_t* d_src, int src_stride, int w, int h, const int32_t* d_src_points, const int32_t* d_src_count,
                                         const SvtHipGmRef* refs, int n_refs, const int32_t* d_ref_points, const int32_t* d_ref_counts, int max_points, int32_t* d_corr,
                                         int32_t* d_ncorr) {
    SVT_HIP_ENTER(c);
    bool bad = !c || gm_plane_bad(d_src, src_stride, w, h) || !d_src_points || !d_src_count || !refs || n_refs < 1 || n_refs > SVT_HIP_GM_MAX_REFS || !d_ref_points ||
               !d_ref_counts || max_points < 1 || max_points > SVT_HIP_GM_MAX_CORNERS || !d_corr || !d_ncorr;
    for (int i = 0; i < n_refs && !bad; i++) bad = !refs[i].d_plane || refs[i].stride < w;   // read as w x h, like the reference: width / height are not used
    if (bad)
        return bad_arg(c, "svt_hip_gm_correspondences_batch_dev: bad argument (source 8 .. 16384 wide and high, every stride >= w, 1 <= n_refs <= 8, 1 <= max_points <= 4096)");
    return launched(c, svt_hip_launch_gm_correspondences(c->stream, d_src, src_stride, w, h, d_src_points, d_src_count, refs, n_refs, d_ref_points, d_ref_counts, max_points,
                                                         d_corr, d_ncorr), "global-motion correspondence launch");
}

/* the model fit (gm_fit.hip) */
size_t svt_hip_gm_fit_scratch_bytes(int njobs, int max_points) {
    if (njobs < 0 || njobs > SVT_HIP_GM_FIT_MAX_JOBS || max_points < 1 || max_points > SVT_HIP_GM_MAX_CORNERS) return 0;
    return svt_hip_gm_fit_scratch_layout_bytes(njobs, max_points);
}

int svt_hip_gm_fit_batch_dev(SvtHipCtx* c, const int32_t* d_corr, const int32_t* d_ncorr, int n_lists, int max_points, const SvtHipGmFitJob* jobs, int njobs,
                             int num_motions, int n_refinements, SvtHipGmFit* d_fits, int32_t* d_inliers, SvtHipGmJob* d_refine_jobs, void* d_scratch) {
    SVT_HIP_ENTER(c);
    if (c && num_motions != 1) return bad_arg(c, "svt_hip_gm_fit_batch_dev: num_motions must be 1 (RANSAC_NUM_MOTIONS)");
    bool bad = !c || num_motions != 1 || !d_corr || !d_ncorr || n_lists < 1 || n_lists > SVT_HIP_GM_MAX_REFS || max_points < 1 || max_points > SVT_HIP_GM_MAX_CORNERS ||
               !jobs || njobs < 0 || njobs > SVT_HIP_GM_FIT_MAX_JOBS || n_refinements < 0 || n_refinements > SVT_HIP_GM_MAX_REFINEMENTS || !d_fits || !d_scratch ||
               ((uintptr_t)d_scratch & 7);
    for (int i = 0; i < njobs && !bad; i++) bad = jobs[i].ref < 0 || jobs[i].ref >= n_lists || jobs[i].type < 1 || jobs[i].type > 3;
    if (bad)
        return bad_arg(c, "svt_hip_gm_fit_batch_dev: bad argument (1 <= n_lists <= 8, 1 <= max_points <= 4096, 0 <= njobs <= 64, every job's 0 <= ref < n_lists and "
                          "1 <= type <= 3, 0 <= n_refinements <= 12, scratch 8-byte aligned)");
    if (!njobs) return SVT_HIP_OK;
    return launched(c, svt_hip_launch_gm_fit(c->stream, d_corr, d_ncorr, max_points, jobs, njobs, n_refinements, d_fits, d_inliers, d_refine_jobs, d_scratch),
                    "global-motion model fit launch");
}

/* the picture call: corners -> correspondences -> fits -> refinement -> frame errors on one stream, one download, the decision on the host */
namespace {
struct GmEstimateLayout {
    size_t points, counts, corners, corr, ncorr, fit_scratch, jobs, refine_scratch, out, fits, results, ferr, out_bytes, total;
    int njobs, nm;
};
size_t gm_up256(size_t v) { return (v + 255) & ~(size_t)255; }
bool gm_estimate_options_bad(const SvtHipGmEstimateOptions* o) {
    return !o || o->max_points < 1 || o->max_points > SVT_HIP_GM_MAX_CORNERS || o->n_refinements < 0 || o->n_refinements > SVT_HIP_GM_MAX_REFINEMENTS;
}
GmEstimateLayout gm_estimate_layout(int w, int h, int n_refs, const SvtHipGmEstimateOptions* o) {
    GmEstimateLayout l = {};
    l.nm = o->rotzoom_model_only ? 1 : 2;
    l.njobs = n_refs * l.nm;
    SvtHipGmRef planes[1 + SVT_HIP_GM_MAX_REFS] = {};
    for (int i = 0; i <= n_refs; i++) { planes[i].width = w; planes[i].height = h; }
    size_t off = 0;
    l.points = off; off += gm_up256((size_t)(1 + n_refs) * o->max_points * 2 * sizeof(int32_t));
    l.counts = off; off += gm_up256((size_t)(1 + n_refs) * sizeof(int32_t));
    l.corners = off; off += gm_up256(svt_hip_gm_corners_scratch_layout_bytes(planes, 1 + n_refs));
    l.corr = off; off += gm_up256((size_t)n_refs * o->max_points * 4 * sizeof(int32_t));
    l.ncorr = off; off += gm_up256((size_t)n_refs * sizeof(int32_t));
    l.fit_scratch = off; off += gm_up256(svt_hip_gm_fit_scratch_layout_bytes(l.njobs, o->max_points));
    l.jobs = off; off += gm_up256((size_t)l.njobs * sizeof(SvtHipGmJob));
    l.refine_scratch = off; off += gm_up256(svt_hip_gm_refine_scratch_layout_bytes(l.njobs));
    l.out = off;   // what the one download takes: fits, refinement results, frame errors, correspondence counts
    l.fits = 0;
    l.results = l.fits + (size_t)l.njobs * sizeof(SvtHipGmFit);
    l.ferr = l.results + (size_t)l.njobs * sizeof(SvtHipGmResult);
    l.out_bytes = l.ferr + (size_t)n_refs * sizeof(int64_t);
    l.total = off + gm_up256(l.out_bytes);
    return l;
}
}  // namespace

size_t svt_hip_gm_estimate_scratch_bytes(int w, int h, int n_refs, const SvtHipGmEstimateOptions* options) {
    if (w < 8 || h < 8 || w > SVT_HIP_GM_MAX_DIM || h > SVT_HIP_GM_MAX_DIM || n_refs < 1 || n_refs > SVT_HIP_GM_MAX_REFS || gm_estimate_options_bad(options)) return 0;
    return gm_estimate_layout(w, h, n_refs, options).total;
}

int svt_hip_gm_estimate_picture_dev(SvtHipCtx* c, const uint8_t* d_src, int stride, int w, int h, const SvtHipGmRef* refs, int n_refs,
                                    const SvtHipGmEstimateOptions* options, SvtHipGmEstimate* results, void* d_scratch) {
    SVT_HIP_ENTER(c);
    bool bad = !c || gm_plane_bad(d_src, stride, w, h) || !refs || n_refs < 1 || n_refs > SVT_HIP_GM_MAX_REFS || gm_estimate_options_bad(options) || !results ||
               !d_scratch || ((uintptr_t)d_scratch & 255);
    // corners and correspondences read a reference over the source's w x h, as the reference does; the refinement clamps to the plane's own size
    for (int i = 0; i < n_refs && !bad; i++)
        bad = gm_plane_bad(refs[i].d_plane, refs[i].stride, refs[i].width, refs[i].height) || refs[i].width < w || refs[i].height < h;
    if (bad)
        return bad_arg(c, "svt_hip_gm_estimate_picture_dev: bad argument (planes 8 .. 16384 wide and high, stride >= width, every reference at least w x h, "
                          "1 <= n_refs <= 8, 1 <= max_points <= 4096, 0 <= n_refinements <= 12, scratch 256-byte aligned)");
    const GmEstimateLayout l = gm_estimate_layout(w, h, n_refs, options);
    uint8_t* base = (uint8_t*)d_scratch;
    int32_t* d_points = (int32_t*)(base + l.points);
    int32_t* d_counts = (int32_t*)(base + l.counts);
    int32_t* d_corr = (int32_t*)(base + l.corr);
    int32_t* d_ncorr = (int32_t*)(base + l.ncorr);
    SvtHipGmJob* d_jobs = (SvtHipGmJob*)(base + l.jobs);
    uint8_t* d_out = base + l.out;
    SvtHipGmFit* d_fits = (SvtHipGmFit*)(d_out + l.fits);
    SvtHipGmResult* d_results = (SvtHipGmResult*)(d_out + l.results);
    int64_t* d_ferr = (int64_t*)(d_out + l.ferr);
    const int mp = options->max_points;

    SvtHipGmRef planes[1 + SVT_HIP_GM_MAX_REFS];
    planes[0] = SvtHipGmRef{d_src, w, h, stride, 0};
    for (int i = 0; i < n_refs; i++) planes[1 + i] = SvtHipGmRef{refs[i].d_plane, w, h, refs[i].stride, 0};
    if (int rc = svt_hip_gm_corners_batch_dev(c, planes, 1 + n_refs, mp, d_points, d_counts, nullptr, base + l.corners)) return rc;
    if (int rc = svt_hip_gm_correspondences_batch_dev(c, d_src, stride, w, h, d_points, d_counts, refs, n_refs, d_points + (size_t)mp * 2, d_counts + 1, mp, d_corr, d_ncorr))
        return rc;
    SvtHipGmFitJob fit_jobs[2 * SVT_HIP_GM_MAX_REFS];
    for (int r = 0; r < n_refs; r++)
        for (int m = 0; m < l.nm; m++) fit_jobs[r * l.nm + m] = SvtHipGmFitJob{r, 2 + m};
    if (int rc = svt_hip_gm_fit_batch_dev(c, d_corr, d_ncorr, n_refs, mp, fit_jobs, l.njobs, 1, options->n_refinements, d_fits, nullptr, d_jobs, base + l.fit_scratch)) return rc;
    if (int rc = svt_hip_gm_frame_error_batch_dev(c, d_src, stride, w, h, refs, n_refs, d_ferr)) return rc;
    if (int rc = svt_hip_gm_refine_picture_dev(c, d_src, stride, w, h, refs, n_refs, d_jobs, l.njobs, d_results, base + l.refine_scratch, nullptr)) return rc;

    std::vector<uint8_t> host(l.out_bytes);
    HIPCHK(c, hipMemcpyAsync(host.data(), d_out, l.out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const SvtHipGmFit* fits = (const SvtHipGmFit*)(host.data() + l.fits);
    const SvtHipGmResult* res = (const SvtHipGmResult*)(host.data() + l.results);
    const int64_t* ferr = (const int64_t*)(host.data() + l.ferr);
    for (int r = 0; r < n_refs; r++) {
        SvtHipGmEstimate* e = results + r;
        std::memset(e, 0, sizeof(*e));
        e->ref_frame_error = ferr[r];
        e->n_models = l.nm;
        for (int m = 0; m < l.nm; m++) {
            const int j = r * l.nm + m;
            e->fits[m] = fits[j];
            SvtHipGmModelRecord* rec = e->models + m;
            rec->num_inliers_kept = fits[j].num_inliers_kept;
            rec->fit_wmtype = fits[j].wmtype;
            for (int k = 0; k < 8; k++) rec->wmmat[k] = res[j].wmmat[k];
            rec->wmtype = res[j].wmtype;
            rec->best_error = res[j].best_error;
        }
        e->num_correspondences = fits[r * l.nm].npoints;
        if (int rc = svt_hip_gm_decide_host(e->models, e->ref_frame_error, options->rotzoom_model_only, options->allow_high_precision_mv, e->wmmat, &e->wmtype)) return rc;
    }
    return SVT_HIP_OK;
}

/* ------------------------------------------------------------------------------------------- ME */
int svt_hip_me_set_waves_per_sb(SvtHipCtx* c, int waves) {
    SVT_HIP_ENTER(c);
    const int w = waves & 15;   // bits 4.. = KiB of LDS padding (experimental single-workgroup-per-CU mode, see me_fullpel.hip)
    if (!c || (w != 1 && w != 2 && w != 4) || (waves >> 4) > 120) return bad_arg(c);
    c->me_waves = waves;
    return SVT_HIP_OK;
}

int svt_hip_me_set_big_windows(SvtHipCtx* c, int enable) {
    SVT_HIP_ENTER(c);
    if (!c) return bad_arg(c);
    c->me_big = enable != 0;
    return SVT_HIP_OK;
}

int svt_hip_me_get_big_windows(SvtHipCtx* c, int* enabled) {
    if (!c || !enabled) return bad_arg(c);
    *enabled = c->me_big;
    return SVT_HIP_OK;
}

int svt_hip_me_fullpel_frame_dev(SvtHipCtx* c, const uint8_t* d_src, const uint8_t* d_ref, int stride, int org_x,
                                 int org_y, const SvtHipSbSearch* d_sbs, int n_sb, int sub_sad, uint32_t* d_best_sad,
                                 uint32_t* d_best_mv) {
    SVT_HIP_ENTER(c);
    if (!c || !d_src || !d_ref || !d_sbs || !d_best_sad || !d_best_mv || n_sb < 0 || (stride & 3))
        return bad_arg(c, "svt_hip_me_fullpel_frame_dev: bad argument (stride must be a multiple of 4)");
    return launched(c, svt_hip_launch_me_fullpel(c->stream, d_src, d_ref, stride, org_x, org_y, d_sbs, n_sb, sub_sad, d_best_sad, d_best_mv, c->me_waves, c->me_big),
                    "me_fullpel launch");
}

int svt_hip_me_fullpel_frame(SvtHipCtx* c, const uint8_t* src, const uint8_t* ref, int stride, int plane_rows, int org_x,
                             int org_y, const SvtHipSbSearch* sbs, int n_sb, int sub_sad, uint32_t* best_sad,
                             uint32_t* best_mv) {
    SVT_HIP_ENTER(c);
    if (!c || !src || !ref || !sbs || !best_sad || !best_mv || n_sb < 0 || plane_rows <= 0) return bad_arg(c);
    int big = 0;
    for (int i = 0; i < n_sb; i++) {
        if (sbs[i].width < 0 || sbs[i].height < 0) return bad_arg(c, "svt_hip_me_fullpel_frame: negative search area");
        big |= (int)sbs[i].width * (int)sbs[i].height > 65536;
    }
    if (!n_sb) return SVT_HIP_OK;
    // Only the rows the windows touch travel (an ME segment is a band of superblock rows), into one staging buffer the context keeps:
    // [source rows | reference rows | windows | SADs | MVs].  Both planes are uploaded over the same row range so that one origin serves both.
    int lo = plane_rows, hi = 0;
    for (int i = 0; i < n_sb; i++) {
        const int s0 = org_y + sbs[i].sb_y, r0 = s0 + sbs[i].y_origin;
        lo = std::min(lo, std::min(s0, r0));
        hi = std::max(hi, std::max(s0 + 64, r0 + (int)sbs[i].height + 63));
    }
    lo = std::max(lo, 0);
    hi = std::min(hi, plane_rows);
    if (lo >= hi) { lo = 0; hi = plane_rows; }
    const size_t band = (size_t)stride * (size_t)(hi - lo), nres = (size_t)n_sb * SVT_HIP_SQUARE_PU_COUNT * 4;
    const size_t off_ref = (band + 256 + 255) & ~(size_t)255 /* slack: dword-aligned window loads may run a few bytes past a row */, off_sbs = 2 * off_ref, off_sad = off_sbs + ((sizeof(SvtHipSbSearch) * (size_t)n_sb + 255) & ~(size_t)255);
    const size_t off_mv = off_sad + ((nres + 255) & ~(size_t)255), total = off_mv + nres + 256;
    if (c->me_buf_bytes < total) {
        if (c->me_buf) (void)hipFree(c->me_buf);
        c->me_buf = nullptr;
        c->me_buf_bytes = 0;
        const hipError_t e = hipMalloc(&c->me_buf, total + total / 4);
        if (e != hipSuccess) return fail(c, e, "svt_hip_me_fullpel_frame: staging buffer");
        c->me_buf_bytes = total + total / 4;
    }
    uint8_t* const base = (uint8_t*)c->me_buf;
    const int saved_big = c->me_big;
    c->me_big = big;   // the windows are known here: launch the strip-walking instance only when one needs it
    int rc = SVT_HIP_OK;
    if ((rc = svt_hip_memcpy_h2d(c, base, src + (size_t)lo * stride, band)) || (rc = svt_hip_memcpy_h2d(c, base + off_ref, ref + (size_t)lo * stride, band)) ||
        (rc = svt_hip_memcpy_h2d(c, base + off_sbs, sbs, sizeof(SvtHipSbSearch) * (size_t)n_sb)))
        goto done;
    if ((rc = svt_hip_me_fullpel_frame_dev(c, base, base + off_ref, stride, org_x, org_y - lo, (const SvtHipSbSearch*)(base + off_sbs), n_sb, sub_sad,
                                           (uint32_t*)(base + off_sad), (uint32_t*)(base + off_mv))))
        goto done;
    if ((rc = svt_hip_memcpy_d2h(c, best_sad, base + off_sad, nres)) || (rc = svt_hip_memcpy_d2h(c, best_mv, base + off_mv, nres))) goto done;
done:
    c->me_big = saved_big;
    return rc;
}

/* ------------------------------------------------------------------------- transform / quant */
static bool quant_ok(const SvtHipQuantParams& q) {
    return q.variant >= 0 && q.variant <= 3 && q.log_scale >= 0 && q.log_scale <= 2 && q.coeff_shape >= 0 && q.coeff_shape <= 3;
}
int svt_hip_fwd_txfm_quant_batch_dev(SvtHipCtx* c, int tx_size, int pix_bytes, const void* d_src, int src_stride,
                                     const void* d_pred, int pred_stride, const uint32_t* d_descs, int nblk,
                                     const SvtHipQuantParams* qp, const SvtHipScanTables* scans, int32_t* d_coeff,
                                     int32_t* d_qcoeff, int32_t* d_dqcoeff, uint16_t* d_eob, int32_t* d_cul_level,
                                     uint64_t* d_energy) {
    SVT_HIP_ENTER(c);
    if (!c || !d_src || !d_pred || !d_descs || nblk < 0 || tx_size < 0 || tx_size > 18 || !pix_ok(pix_bytes) ||
        ((d_qcoeff != nullptr) != (d_dqcoeff != nullptr)) || (d_qcoeff && (!qp || !scans || !scans->iscan[0])) || (qp && !quant_ok(*qp)))
        return bad_arg(c, "svt_hip_fwd_txfm_quant_batch_dev: bad argument");
    return launched(c, svt_hip_launch_fwd_txfm_quant(c->stream, tx_size, pix_bytes, d_src, src_stride, d_pred, pred_stride, d_descs, nblk, qp, scans, d_coeff, d_qcoeff,
                                                     d_dqcoeff, d_eob, d_cul_level, d_energy), "fwd_txfm_quant launch");
}

int svt_hip_inv_txfm_add_batch_dev(SvtHipCtx* c, int tx_size, int pix_bytes, int bd, const int32_t* d_dqcoeff, const void* d_pred,
                                   int pred_stride, void* d_recon, int recon_stride, const uint32_t* d_descs, int nblk) {
    SVT_HIP_ENTER(c);
    if (!c || !d_dqcoeff || !d_pred || !d_recon || !d_descs || nblk < 0 || tx_size < 0 || tx_size > 18 || !fmt_ok(pix_bytes, bd))
        return bad_arg(c, "svt_hip_inv_txfm_add_batch_dev: bad argument");
    return launched(c, svt_hip_launch_inv_txfm_add(c->stream, tx_size, pix_bytes, bd, d_dqcoeff, d_pred, pred_stride, d_recon, recon_stride, d_descs, nblk), "inv_txfm_add launch");
}

int svt_hip_iwht4x4_add_batch_dev(SvtHipCtx* c, int pix_bytes, int bd, const int32_t* d_dqcoeff, const uint16_t* d_eob, const void* d_pred, int pred_stride,
                                  void* d_recon, int recon_stride, const uint32_t* d_descs, int nblk) {
    SVT_HIP_ENTER(c);
    if (!c || !d_dqcoeff || !d_pred || !d_recon || !d_descs || nblk < 0 || !fmt_ok(pix_bytes, bd) || ((uintptr_t)d_dqcoeff & 15))
        return bad_arg(c, "svt_hip_iwht4x4_add_batch_dev: bad argument");
    return launched(c, svt_hip_launch_iwht4x4_add(c->stream, pix_bytes, bd, d_dqcoeff, d_eob, d_pred, pred_stride, d_recon, recon_stride, d_descs, nblk), "iwht4x4_add launch");
}

/* ------------------------------------------------------------------------------- deblocking */
int svt_hip_deblock_plane_dev(SvtHipCtx* c, void* d_plane, int pix_bytes, int stride, int bd, const uint16_t* d_edges_v,
                              const uint16_t* d_edges_h, int units_w, int units_h, int sharpness) {
    SVT_HIP_ENTER(c);
    if (!c || !d_plane || !fmt_ok(pix_bytes, bd) || units_w < 0 || units_h < 0 || sharpness < 0 || sharpness > 7 || (!d_edges_v && !d_edges_h))
        return bad_arg(c, "svt_hip_deblock_plane_dev: bad argument");
    return launched(c, svt_hip_launch_deblock_plane(c->stream, d_plane, pix_bytes, stride, bd, d_edges_v, d_edges_h, units_w, units_h, sharpness, -1, -1), "deblock launch");
}

int svt_hip_deblock_frame_dev(SvtHipCtx* c, void* const d_plane[3], int pix_bytes, const int stride[3], int bd, const uint16_t* const d_edges_v[3],
                              const uint16_t* const d_edges_h[3], const int units_w[3], const int units_h[3], int sharpness) {
    SVT_HIP_ENTER(c);
    if (!c || !d_plane || !stride || !d_edges_v || !d_edges_h || !units_w || !units_h || !fmt_ok(pix_bytes, bd) || sharpness < 0 || sharpness > 7)
        return bad_arg(c, "svt_hip_deblock_frame_dev: bad argument");
    for (int p = 0; p < 3; p++)
        if (d_plane[p] && (units_w[p] < 0 || units_h[p] < 0 || !d_edges_v[p] || !d_edges_h[p])) return bad_arg(c);
    return launched(c, svt_hip_launch_deblock_frame(c->stream, d_plane, pix_bytes, stride, bd, d_edges_v, d_edges_h, units_w, units_h, sharpness), "deblock frame launch");
}

int svt_hip_deblock_frame_fused_dev(SvtHipCtx* c, const void* const d_src[3], void* const d_dst[3], int pix_bytes, const int stride[3], int bd, const int plane_w[3],
                                    const int plane_h[3], const uint16_t* const d_edges_v[3], const uint16_t* const d_edges_h[3], const int units_w[3],
                                    const int units_h[3], int sharpness) {
    SVT_HIP_ENTER(c);
    if (!c || !d_src || !d_dst || !stride || !plane_w || !plane_h || !d_edges_v || !d_edges_h || !units_w || !units_h || !fmt_ok(pix_bytes, bd) || sharpness < 0 || sharpness > 7)
        return bad_arg(c, "svt_hip_deblock_frame_fused_dev: bad argument");
    for (int p = 0; p < 3; p++)
        if (d_src[p] && (!d_dst[p] || d_dst[p] == d_src[p] || plane_w[p] <= 0 || plane_h[p] <= 0 || units_w[p] < (plane_w[p] + 3) / 4 || units_h[p] < (plane_h[p] + 3) / 4 ||
                         !d_edges_v[p] || !d_edges_h[p]))
            return bad_arg(c, "svt_hip_deblock_frame_fused_dev: bad plane argument (the fused form is out of place)");
    return launched(c, svt_hip_launch_deblock_fused(c->stream, d_src, d_dst, pix_bytes, stride, bd, plane_w, plane_h, d_edges_v, d_edges_h, units_w, units_h, sharpness),
                    "fused deblock launch");
}

int svt_hip_dlf_build_edges_picture_dev(SvtHipCtx* c, const SvtHipDlfModeInfo* d_mi, int mi_cols, int mi_rows, int ss_x, int ss_y, const int plane_w[3], const int plane_h[3],
                                        const int filt_units_w[3], const int filt_units_h[3], const int (*level)[2], uint16_t* const d_edges_v[3], uint16_t* const d_edges_h[3]) {
    SVT_HIP_ENTER(c);
    if (!c || !d_mi || mi_cols <= 0 || mi_rows <= 0 || ss_x < 0 || ss_x > 1 || ss_y < 0 || ss_y > 1 || !plane_w || !plane_h || !filt_units_w || !filt_units_h || !d_edges_v ||
        !d_edges_h)
        return bad_arg(c, "svt_hip_dlf_build_edges_picture_dev: bad argument");
    for (int p = 0; p < 3; p++) {
        if (!d_edges_v[p] && !d_edges_h[p]) continue;
        if (!d_edges_v[p] || !d_edges_h[p] || plane_w[p] <= 0 || plane_h[p] <= 0 || filt_units_w[p] < 0 || filt_units_h[p] < 0 ||
            (level && (level[p][0] > 63 || level[p][1] > 63)))
            return bad_arg(c, "svt_hip_dlf_build_edges_picture_dev: bad plane argument");
    }
    return launched(c, svt_hip_launch_dlf_build_edges(c->stream, d_mi, mi_cols, mi_rows, ss_x, ss_y, plane_w, plane_h, filt_units_w, filt_units_h, level, d_edges_v,
                                                      d_edges_h), "edge builder launch");
}

int svt_hip_plane_sse_dev(SvtHipCtx* c, int pix_bytes, const void* d_a, int a_stride, const void* d_b, int b_stride, int w, int h,
                          uint64_t* d_sse) {
    SVT_HIP_ENTER(c);
    if (!c || !d_a || !d_b || !d_sse || !pix_ok(pix_bytes) || w <= 0 || h <= 0) return bad_arg(c, "svt_hip_plane_sse_dev: bad argument");
    HIPCHK(c, hipMemsetAsync(d_sse, 0, sizeof(uint64_t), c->stream));
    return launched(c, svt_hip_launch_plane_sse(c->stream, pix_bytes, d_a, a_stride, d_b, b_stride, w, h, d_sse), "plane sse launch");
}

// search_filter_level (EbDeblockingFilter.c:1026-1187); every try_filter_frame (:966-1024) runs on the device.
int svt_hip_dlf_search_level_dev(SvtHipCtx* c, const SvtHipDlfSearch* p, const void* d_recon, void* d_tmp, int pix_bytes, int stride,
                                 int bd, int plane_w, int plane_h, const void* d_src, int src_stride, const uint16_t* d_edges_v,
                                 const uint16_t* d_edges_h, int units_w, int units_h, uint64_t* d_sse_scratch, int* best_level,
                                 int64_t* best_err_out) {
    SVT_HIP_ENTER(c);
    if (!c || !p || !d_recon || !d_tmp || !d_src || !d_edges_v || !d_edges_h || !d_sse_scratch || !best_level || p->plane < 0 || p->plane > 2 || !fmt_ok(pix_bytes, bd) ||
        plane_w <= 0 || plane_h <= 0 || units_w != (plane_w + 3) / 4 || units_h != (plane_h + 3) / 4 || p->sharpness < 0 || p->sharpness > 7)
        return bad_arg(c, "svt_hip_dlf_search_level_dev: bad argument");
    int rc = SVT_HIP_OK;
    auto try_level = [&](int lv_v, int lv_h) -> int64_t {   // try_filter_frame (:966-1024) on the device
        uint64_t sse = 0;
        hipError_t e = hipMemcpy2DAsync(d_tmp, (size_t)stride * pix_bytes, d_recon, (size_t)stride * pix_bytes, (size_t)plane_w * pix_bytes,
                                        plane_h, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = (hipError_t)svt_hip_launch_deblock_plane(c->stream, d_tmp, pix_bytes, stride, bd, d_edges_v, d_edges_h, units_w, units_h, p->sharpness, lv_v, lv_h);
        if (e == hipSuccess) e = hipMemsetAsync(d_sse_scratch, 0, sizeof(uint64_t), c->stream);
        if (e == hipSuccess) e = (hipError_t)svt_hip_launch_plane_sse(c->stream, pix_bytes, d_src, src_stride, d_tmp, stride, plane_w, plane_h, d_sse_scratch);
        if (e == hipSuccess) e = hipMemcpyAsync(&sse, d_sse_scratch, sizeof(sse), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { rc = fail(c, e, "dlf level probe"); return -1; }
        return (int64_t)sse;
    };
    struct Thunk { decltype(try_level)* f; } th{&try_level};
    const int hrc = svt_hip_dlf_search_levels_host(p, [](void* u, int lv_v, int lv_h) -> int64_t { return (*((Thunk*)u)->f)(lv_v, lv_h); }, &th,
                                                   best_level, best_err_out);
    return rc != SVT_HIP_OK ? rc : hrc;
}

int svt_hip_dlf_search_levels_picture_dev(SvtHipCtx* c, int n_planes, const SvtHipDlfSearchPlane* planes, int pix_bytes, int bd, uint64_t* d_sse_scratch, int* best_level,
                                          int64_t* best_err) {
    SVT_HIP_ENTER(c);
    if (!c || !planes || n_planes < 1 || n_planes > 3 || !d_sse_scratch || !best_level || !fmt_ok(pix_bytes, bd)) return bad_arg(c);
    for (int i = 0; i < n_planes; i++) {
        const SvtHipDlfSearchPlane& P = planes[i];
        if (!P.d_recon || !P.d_tmp[0] || !P.d_tmp[1] || !P.d_src || !P.d_edges_v || !P.d_edges_h || P.q.plane < 0 || P.q.plane > 2 || P.plane_w <= 0 || P.plane_h <= 0 ||
            P.units_w != (P.plane_w + 3) / 4 || P.units_h != (P.plane_h + 3) / 4 || P.q.sharpness < 0 || P.q.sharpness > 7)
            return bad_arg(c, "svt_hip_dlf_search_levels_picture_dev: bad plane");
    }
    int64_t ss_err[3][64];
    bool    done[3] = {false, false, false};
    for (int i = 0; i < 3; i++) for (int k = 0; k < 64; k++) ss_err[i][k] = -1;
    for (;;) {
        int need[3][2], n_need[3] = {0, 0, 0}, total = 0;
        for (int i = 0; i < n_planes; i++) {
            if (done[i]) continue;
            const int n = svt_hip_dlf_search_plan(&planes[i].q, ss_err[i], need[i], &best_level[i], best_err ? &best_err[i] : nullptr);
            if (n < 0) return n;
            if (n == 0) done[i] = true;
            n_need[i] = n; total += n;
        }
        if (!total) break;
        hipError_t e = hipMemsetAsync(d_sse_scratch, 0, sizeof(uint64_t) * 2 * n_planes, c->stream);
        for (int i = 0; i < n_planes && e == hipSuccess; i++)
            for (int k = 0; k < n_need[i] && e == hipSuccess; k++) {   // try_filter_frame (:966-1024) on the device: a copy of the plane as coded, deblocked at the probed level, against the source
                const SvtHipDlfSearchPlane& P = planes[i];
                int lv_v, lv_h;
                svt_hip_dlf_search_probe_levels(&P.q, need[i][k], &lv_v, &lv_h);
                e = hipMemcpy2DAsync(P.d_tmp[k], (size_t)P.stride * pix_bytes, P.d_recon, (size_t)P.stride * pix_bytes, (size_t)P.plane_w * pix_bytes, P.plane_h, hipMemcpyDeviceToDevice, c->stream);
                if (e == hipSuccess) e = (hipError_t)svt_hip_launch_deblock_plane(c->stream, P.d_tmp[k], pix_bytes, P.stride, bd, P.d_edges_v, P.d_edges_h, P.units_w, P.units_h, P.q.sharpness, lv_v, lv_h);
                if (e == hipSuccess) e = (hipError_t)svt_hip_launch_plane_sse(c->stream, pix_bytes, P.d_src, P.src_stride, P.d_tmp[k], P.stride, P.plane_w, P.plane_h, d_sse_scratch + 2 * i + k);
            }
        uint64_t sse[6] = {0, 0, 0, 0, 0, 0};
        if (e == hipSuccess) e = hipMemcpyAsync(sse, d_sse_scratch, sizeof(uint64_t) * 2 * n_planes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, e, "dlf level probes of a picture");
        for (int i = 0; i < n_planes; i++)
            for (int k = 0; k < n_need[i]; k++) ss_err[i][need[i][k]] = (int64_t)sse[2 * i + k];
    }
    return SVT_HIP_OK;
}

int svt_hip_fwd_txfm_quant_multi_dev(SvtHipCtx* c, int pix_bytes, const SvtHipFwdTxJob* jobs, int njobs) {
    SVT_HIP_ENTER(c);
    if (!c || (!jobs && njobs) || njobs < 0 || !pix_ok(pix_bytes)) return bad_arg(c);
    for (int j = 0; j < njobs; j++) {
        const SvtHipFwdTxJob& J = jobs[j];
        if (J.nblk < 0 || J.tx_size < 0 || J.tx_size > 18 || (J.nblk && (!J.d_src || !J.d_pred || !J.d_descs)) || ((J.d_qcoeff != nullptr) != (J.d_dqcoeff != nullptr)) ||
            (J.d_qcoeff && !J.scans.iscan[0]) || !quant_ok(J.qp))
            return bad_arg(c, "svt_hip_fwd_txfm_quant_multi_dev: bad job");
    }
    return launched(c, svt_hip_launch_fwd_txfm_quant_multi(c->stream, pix_bytes, jobs, njobs), "fwd_txfm_quant multi launch");
}
int svt_hip_enc_txfm_multi_dev(SvtHipCtx* c, int pix_bytes, int bd, const SvtHipEncTxJob* jobs, int njobs) {
    SVT_HIP_ENTER(c);
    if (!c || (!jobs && njobs) || njobs < 0 || !fmt_ok(pix_bytes, bd)) return bad_arg(c);
    for (int j = 0; j < njobs; j++) {
        const SvtHipFwdTxJob& J = jobs[j].fwd;
        if (J.nblk < 0 || J.tx_size < 0 || J.tx_size > 18 || (J.nblk && (!J.d_src || !J.d_pred || !J.d_descs || !J.d_qcoeff || !jobs[j].d_recon || !J.scans.iscan[0])) ||
            !quant_ok(J.qp))
            return bad_arg(c, "svt_hip_enc_txfm_multi_dev: bad job");
    }
    return launched(c, svt_hip_launch_enc_txfm_multi(c->stream, pix_bytes, bd, jobs, njobs), "encode transform multi launch");
}
int svt_hip_inv_txfm_add_multi_dev(SvtHipCtx* c, int pix_bytes, int bd, const SvtHipInvTxJob* jobs, int njobs) {
    SVT_HIP_ENTER(c);
    if (!c || (!jobs && njobs) || njobs < 0 || !fmt_ok(pix_bytes, bd)) return bad_arg(c);
    for (int j = 0; j < njobs; j++) {
        const SvtHipInvTxJob& J = jobs[j];
        if (J.nblk < 0 || J.tx_size < 0 || J.tx_size > 18 || (J.nblk && (!J.d_dqcoeff || !J.d_pred || !J.d_recon || !J.d_descs)))
            return bad_arg(c, "svt_hip_inv_txfm_add_multi_dev: bad job");
    }
    return launched(c, svt_hip_launch_inv_txfm_add_multi(c->stream, pix_bytes, bd, jobs, njobs), "inv_txfm_add multi launch");
}

/* ------------------------------------------------------------------------------------- CDEF */
int svt_hip_cdef_search_frame_dev(SvtHipCtx* c, int pix_bytes, const void* const d_rec[3], const int rec_stride[3],
                                  const void* const d_src[3], const int src_stride[3], int w, int h, const uint8_t* d_skip8,
                                  int pri_damping, int bd, uint64_t* d_mse, uint8_t* d_dir, int32_t* d_var) {
    SVT_HIP_ENTER(c);
    if (!c || !d_rec || !d_src || !rec_stride || !src_stride || !d_skip8 || !d_mse || !d_dir || !d_var || !fmt_ok(pix_bytes, bd) || w <= 0 || h <= 0 || (w & 7) || (h & 7))
        return bad_arg(c, "svt_hip_cdef_search_frame_dev: bad argument");
    return launched(c, svt_hip_launch_cdef_search(c->stream, pix_bytes, d_rec, rec_stride, d_src, src_stride, w, h, d_skip8, pri_damping, bd, d_mse, d_dir, d_var),
                    "cdef search launch");
}
int svt_hip_cdef_apply_frame_dev(SvtHipCtx* c, int pix_bytes, const void* const d_in[3], void* const d_out[3], const int stride[3], int w,
                                 int h, const uint8_t* d_skip8, const uint8_t* d_y_strength, const uint8_t* d_uv_strength, int damping,
                                 int bd, uint8_t* d_dir, const int32_t* d_var) {
    SVT_HIP_ENTER(c);
    if (!c || !d_in || !d_out || !stride || !d_skip8 || !d_y_strength || !d_uv_strength || !d_dir || !fmt_ok(pix_bytes, bd) || w <= 0 || h <= 0 || (w & 7) || (h & 7))
        return bad_arg(c, "svt_hip_cdef_apply_frame_dev: bad argument");
    return launched(c, svt_hip_launch_cdef_apply(c->stream, pix_bytes, d_in, d_out, stride, w, h, d_skip8, d_y_strength, d_uv_strength, damping, bd, d_dir, d_var),
                    "cdef apply launch");
}

/* -------------------------------------------------------------- sub-pel predict / SAD / variance */
int svt_hip_subpel_predict_batch_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_ref, int ref_stride, void* d_dst, int dst_stride,
                                     const SvtHipConvBlk* d_blks, int nblk) {
    SVT_HIP_ENTER(c);
    if (!c || !d_ref || !d_dst || !d_blks || nblk < 0 || !fmt_ok(pix_bytes, bd)) return bad_arg(c, "svt_hip_subpel_predict_batch_dev: bad argument");
    return launched(c, svt_hip_launch_subpel_predict(c->stream, pix_bytes, bd, d_ref, ref_stride, d_dst, dst_stride, d_blks, nblk), "subpel predict launch");
}
int svt_hip_subpel_jobs_from_me_dev(SvtHipCtx* c, const uint32_t* d_best_mv, int sb_cols, int w, int h, const uint8_t* d_frac_q4, SvtHipConvBlk* d_blks) {
    SVT_HIP_ENTER(c);
    if (!c || !d_best_mv || !d_blks || sb_cols < 1 || w < 16 || h < 16 || (w + 63) / 64 > sb_cols) return bad_arg(c);
    return launched(c, svt_hip_launch_subpel_jobs_from_me(c->stream, d_best_mv, sb_cols, w, h, d_frac_q4, d_blks), "subpel jobs launch");
}
int svt_hip_block_sad_batch_dev(SvtHipCtx* c, int pix_bytes, const void* d_a, int a_stride, const void* d_b, int b_stride,
                                const SvtHipBlkPair* d_pairs, int n, uint32_t* d_sad) {
    SVT_HIP_ENTER(c);
    if (!c || !d_a || !d_b || !d_pairs || !d_sad || n < 0 || !pix_ok(pix_bytes)) return bad_arg(c);
    return launched(c, svt_hip_launch_block_sad(c->stream, pix_bytes, d_a, a_stride, d_b, b_stride, d_pairs, n, d_sad), "block sad launch");
}
// What the md_*_picture forms share: the picture's geometry, the prediction-unit list and the reference-plane list.  The SAD forms also bound every unit's own
// width and height; the grid forms take any unit that lies inside the superblock.
static bool md_picture_ok(const void* d_src, const uint32_t* d_mv, const uint32_t* d_out, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus, const SvtHipMdPu* pus, int n_refs,
                          const SvtHipMdRefPlane* refs, bool sad_units) {
    if (!d_src || !pus || !refs || !d_mv || !d_out || n_sb < 0 || sb_cols < 1 || pic_w < 1 || pic_h < 1 || n_pus < 1 || n_pus > SVT_HIP_MD_MAX_PUS || n_refs < 1 ||
        n_refs > SVT_HIP_MD_MAX_REFS)
        return false;
    for (int i = 0; i < n_pus; i++) {
        if (sad_units && (pus[i].w < 4 || pus[i].w > 64 || (pus[i].w & 3) || pus[i].h < 1 || pus[i].h > 64)) return false;
        if (pus[i].x + pus[i].w > 64 || pus[i].y + pus[i].h > 64) return false;
    }
    for (int i = 0; i < n_refs; i++)
        if (!refs[i].d_plane || refs[i].stride < 1) return false;
    return true;
}
static int md_sad_picture(int pix_bytes, SvtHipCtx* c, const void* d_src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus, const SvtHipMdPu* pus,
                          int n_refs, const SvtHipMdRefPlane* refs, const uint32_t* d_mv, uint32_t* d_sad) {
    if (!c || !md_picture_ok(d_src, d_mv, d_sad, pic_w, pic_h, sb_cols, n_sb, n_pus, pus, n_refs, refs, true)) return bad_arg(c);
    return launched(c, svt_hip_launch_md_fullpel_sad(c->stream, pix_bytes, d_src, src_stride, pic_w, pic_h, sb_cols, n_sb, n_pus, pus, n_refs, refs, d_mv, d_sad),
                    "md full-pel sad launch");
}
int svt_hip_md_fullpel_sad_picture_dev(SvtHipCtx* c, const uint8_t* d_src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus, const SvtHipMdPu* pus,
                                       int n_refs, const SvtHipMdRefPlane* refs, const uint32_t* d_mv, uint32_t* d_sad) {
    SVT_HIP_ENTER(c);
    return md_sad_picture(1, c, d_src, src_stride, pic_w, pic_h, sb_cols, n_sb, n_pus, pus, n_refs, refs, d_mv, d_sad);
}
int svt_hip_md_fullpel_sad_picture_hbd_dev(SvtHipCtx* c, const uint16_t* d_src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus, const SvtHipMdPu* pus,
                                           int n_refs, const SvtHipMdRefPlane* refs, const uint32_t* d_mv, uint32_t* d_sad) {
    SVT_HIP_ENTER(c);
    return md_sad_picture(2, c, d_src, src_stride, pic_w, pic_h, sb_cols, n_sb, n_pus, pus, n_refs, refs, d_mv, d_sad);
}
static int md_avg_sad_picture(int pix_bytes, SvtHipCtx* c, const void* d_src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus, const SvtHipMdPu* pus,
                              int n_refs, const SvtHipMdRefPlane* refs, const uint32_t* d_mv, int n_pairs, const uint8_t (*pairs)[2], uint32_t* d_sad) {
    if (!c || !md_picture_ok(d_src, d_mv, d_sad, pic_w, pic_h, sb_cols, n_sb, n_pus, pus, n_refs, refs, true) || !pairs || n_pairs < 1 || n_pairs > SVT_HIP_MD_MAX_PAIRS)
        return bad_arg(c);
    for (int i = 0; i < n_pairs; i++)
        if (pairs[i][0] >= n_refs || pairs[i][1] >= n_refs) return bad_arg(c);
    return launched(c, svt_hip_launch_md_fullpel_avg_sad(c->stream, pix_bytes, d_src, src_stride, pic_w, pic_h, sb_cols, n_sb, n_pus, pus, n_refs, refs, d_mv, n_pairs,
                                                         pairs, d_sad), "md compound-average sad launch");
}
int svt_hip_md_fullpel_avg_sad_picture_dev(SvtHipCtx* c, const uint8_t* d_src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus, const SvtHipMdPu* pus,
                                           int n_refs, const SvtHipMdRefPlane* refs, const uint32_t* d_mv, int n_pairs, const uint8_t (*pairs)[2], uint32_t* d_sad) {
    SVT_HIP_ENTER(c);
    return md_avg_sad_picture(1, c, d_src, src_stride, pic_w, pic_h, sb_cols, n_sb, n_pus, pus, n_refs, refs, d_mv, n_pairs, pairs, d_sad);
}
int svt_hip_md_fullpel_avg_sad_picture_hbd_dev(SvtHipCtx* c, const uint16_t* d_src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus, const SvtHipMdPu* pus,
                                               int n_refs, const SvtHipMdRefPlane* refs, const uint32_t* d_mv, int n_pairs, const uint8_t (*pairs)[2], uint32_t* d_sad) {
    SVT_HIP_ENTER(c);
    return md_avg_sad_picture(2, c, d_src, src_stride, pic_w, pic_h, sb_cols, n_sb, n_pus, pus, n_refs, refs, d_mv, n_pairs, pairs, d_sad);
}
static int md_grid_picture(int grid, SvtHipCtx* c, const uint8_t* d_src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus, const SvtHipMdPu* pus,
                           int n_refs, const SvtHipMdRefPlane* refs, const uint32_t* d_mv, int bank, uint32_t* d_out) {
    if (!c || !md_picture_ok(d_src, d_mv, d_out, pic_w, pic_h, sb_cols, n_sb, n_pus, pus, n_refs, refs, false) || bank < 0 || bank > 5) return bad_arg(c);
    return launched(c, svt_hip_launch_md_subpel_grid(c->stream, d_src, src_stride, pic_w, pic_h, sb_cols, n_sb, n_pus, pus, n_refs, refs, d_mv, bank, grid, d_out),
                    "md sub-pel grid launch");
}
int svt_hip_md_subpel_grid_picture_dev(SvtHipCtx* c, const uint8_t* d_src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus, const SvtHipMdPu* pus,
                                       int n_refs, const SvtHipMdRefPlane* refs, const uint32_t* d_mv, int bank, uint32_t* d_out) {
    SVT_HIP_ENTER(c);
    return md_grid_picture(7, c, d_src, src_stride, pic_w, pic_h, sb_cols, n_sb, n_pus, pus, n_refs, refs, d_mv, bank, d_out);
}
int svt_hip_md_halfpel_grid_picture_dev(SvtHipCtx* c, const uint8_t* d_src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus, const SvtHipMdPu* pus,
                                        int n_refs, const SvtHipMdRefPlane* refs, const uint32_t* d_mv, int bank, uint32_t* d_out) {
    SVT_HIP_ENTER(c);
    return md_grid_picture(3, c, d_src, src_stride, pic_w, pic_h, sb_cols, n_sb, n_pus, pus, n_refs, refs, d_mv, bank, d_out);
}
int svt_hip_coeff_distortion_batch_dev(SvtHipCtx* c, const int32_t* d_coeff, const int32_t* d_recon_coeff, int n_per_block, int nblk, uint64_t* d_out) {
    SVT_HIP_ENTER(c);
    if (!c || !d_coeff || !d_out || n_per_block <= 0 || nblk < 0) return bad_arg(c);
    return launched(c, svt_hip_launch_coeff_distortion(c->stream, d_coeff, d_recon_coeff, n_per_block, nblk, d_out), "coeff distortion launch");
}
int svt_hip_block_sse_batch_dev(SvtHipCtx* c, int pix_bytes, const void* d_a, int a_stride, const void* d_b, int b_stride, const SvtHipBlkPair* d_pairs,
                                int n, uint64_t* d_sse) {
    SVT_HIP_ENTER(c);
    if (!c || !d_a || !d_b || !d_pairs || !d_sse || n < 0 || !pix_ok(pix_bytes)) return bad_arg(c);
    return launched(c, svt_hip_launch_block_sse(c->stream, pix_bytes, d_a, a_stride, d_b, b_stride, d_pairs, n, d_sse), "block sse launch");
}
int svt_hip_block_variance_batch_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_a, int a_stride, const void* d_b, int b_stride,
                                     const SvtHipBlkPair* d_pairs, int n, uint32_t* d_var, uint32_t* d_sse) {
    SVT_HIP_ENTER(c);
    if (!c || !d_a || !d_b || !d_pairs || !d_var || n < 0 || !((pix_bytes == 1 && bd == 8) || (pix_bytes == 2 && (bd == 10 || bd == 16)))) return bad_arg(c);
    return launched(c, svt_hip_launch_block_variance(c->stream, pix_bytes, bd, d_a, a_stride, d_b, b_stride, d_pairs, n, d_var, d_sse), "block variance launch");
}

/* ------------------------------------------------------------------- pyramids / HME search */
int svt_hip_downsample_2d_dev(SvtHipCtx* c, const uint8_t* d_in, int in_stride, int w, int h, uint8_t* d_out, int out_stride, int step,
                              int filtered) {
    SVT_HIP_ENTER(c);
    if (!c || !d_in || !d_out || (step != 2 && step != 4) || w < step || h < step) return bad_arg(c);
    return launched(c, svt_hip_launch_downsample(c->stream, d_in, in_stride, w, h, d_out, out_stride, step, filtered), "downsample launch");
}
int svt_hip_variance_pyramid_dev(SvtHipCtx* c, const uint8_t* d_plane, int stride, int sb_cols, int n_sb, int full_precision,
                                 uint8_t* d_mean, uint16_t* d_var) {
    SVT_HIP_ENTER(c);
    if (!c || !d_plane || !d_mean || !d_var || sb_cols <= 0 || n_sb < 0 || (stride & 7) || ((uintptr_t)d_plane & 7))
        return bad_arg(c, "svt_hip_variance_pyramid_dev: bad argument (plane and stride must be 8-byte aligned)");
    return launched(c, svt_hip_launch_variance_pyramid(c->stream, d_plane, stride, sb_cols, n_sb, full_precision, d_mean, d_var), "variance pyramid launch");
}
int svt_hip_sad_loop_batch_dev(SvtHipCtx* c, const uint8_t* d_src, int src_stride, const uint8_t* d_ref, int ref_stride,
                               const SvtHipSadLoop* d_searches, int n, uint32_t* d_best_sad, int16_t* d_best_xy) {
    SVT_HIP_ENTER(c);
    if (!c || !d_src || !d_ref || !d_searches || !d_best_sad || !d_best_xy || n < 0) return bad_arg(c);
    return launched(c, svt_hip_launch_sad_loop(c->stream, d_src, src_stride, d_ref, ref_stride, d_searches, n, d_best_sad, d_best_xy), "sad loop launch");
}

int svt_hip_sad_loop16_batch_dev(SvtHipCtx* c, const uint16_t* d_src, int src_stride, const uint16_t* d_ref, int ref_stride, const SvtHipSadLoop* d_searches, int n,
                                 uint32_t* d_best_sad, int16_t* d_best_xy) {
    SVT_HIP_ENTER(c);
    if (!c || n < 0) return bad_arg(c);
    if (n == 0) return SVT_HIP_OK;
    if (!d_src || !d_ref || !d_searches || !d_best_sad || !d_best_xy) return bad_arg(c);
    return launched(c, svt_hip_launch_sad_loop16(c->stream, d_src, src_stride, d_ref, ref_stride, d_searches, n, d_best_sad, d_best_xy), "sad loop (16-bit) launch");
}

/* ---------------------------------------------------------------- self-guided restoration */
static bool sgr_args_ok(int pix_bytes, int bd, int pw, int ph) { return fmt_ok(pix_bytes, bd) && pw > 0 && ph > 0; }
// ... and the restoration units of the plane: a multiple of 64 wide, luma or vertically subsampled chroma
static bool lr_plane_ok(int pix_bytes, int bd, int pw, int ph, int unit_size, int ss_y) {
    return sgr_args_ok(pix_bytes, bd, pw, ph) && unit_size >= 64 && !(unit_size & 63) && (ss_y == 0 || ss_y == 1);
}
static int sgr_units(int size, int unit) { const int n = (size + unit / 2) / unit; return n > 0 ? n : 1; }
// The library-owned device scratch only grows.  It may still be in use by work queued on ANY stream this context was pointed at.
static int grow_scratch(SvtHipCtx* c, size_t need) {
    if (need <= c->scratch_bytes) return SVT_HIP_OK;
    HIPCHK(c, hipDeviceSynchronize());
    if (c->scratch) HIPCHK(c, hipFree(c->scratch));
    c->scratch = nullptr; c->scratch_bytes = 0;
    HIPCHK(c, hipMalloc(&c->scratch, need));
    c->scratch_bytes = need;
    return SVT_HIP_OK;
}

int svt_hip_sgr_filter_plane_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_plane, int stride, int pw, int ph, int ep,
                                 int32_t* d_flt0, int32_t* d_flt1, int flt_stride) {
    SVT_HIP_ENTER(c);
    if (!c || !d_plane || !d_flt0 || !d_flt1 || ep < 0 || ep > 15 || !sgr_args_ok(pix_bytes, bd, pw, ph)) return bad_arg(c);
    return launched(c, svt_hip_launch_sgr_filter(c->stream, pix_bytes, bd, d_plane, stride, pw, ph, ep, d_flt0, d_flt1, flt_stride), "sgr filter launch");
}
int svt_hip_sgr_search_plane_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_dgd, int stride, const void* d_src, int src_stride,
                                 int pw, int ph, int unit_size, int ss_y, uint32_t ep_mask, int64_t* d_sums) {
    SVT_HIP_ENTER(c);
    if (!c || !d_dgd || !d_src || !d_sums || !lr_plane_ok(pix_bytes, bd, pw, ph, unit_size, ss_y)) return bad_arg(c);
    return launched(c, svt_hip_launch_sgr_search(c->stream, pix_bytes, bd, d_dgd, stride, d_src, src_stride, pw, ph, unit_size, sgr_units(pw, unit_size),
                                                 sgr_units(ph, unit_size), ss_y, ep_mask & 0xFFFFu, d_sums), "sgr search launch");
}
int svt_hip_sgr_apply_plane_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_dgd, int stride, void* d_dst, int dst_stride, int pw,
                                int ph, int unit_size, int ss_y, const void* d_dbl, int dbl_stride, const uint8_t* d_unit_ep,
                                const int32_t* d_unit_xqd) {
    SVT_HIP_ENTER(c);
    return svt_hip_lr_apply_plane_dev(c, pix_bytes, bd, d_dgd, stride, d_dst, dst_stride, pw, ph, unit_size, ss_y, d_dbl, dbl_stride, d_unit_ep,
                                      d_unit_xqd, nullptr);
}
int svt_hip_lr_apply_plane_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_dgd, int stride, void* d_dst, int dst_stride, int pw, int ph,
                               int unit_size, int ss_y, const void* d_dbl, int dbl_stride, const uint8_t* d_unit_ep, const int32_t* d_unit_xqd,
                               const int16_t* d_unit_wiener) {
    SVT_HIP_ENTER(c);
    if (!c || !d_dgd || !d_dst || !d_unit_ep || !d_unit_xqd || !lr_plane_ok(pix_bytes, bd, pw, ph, unit_size, ss_y)) return bad_arg(c);
    return launched(c, svt_hip_launch_sgr_apply(c->stream, pix_bytes, bd, d_dgd, stride, d_dst, dst_stride, pw, ph, unit_size, sgr_units(pw, unit_size),
                                                sgr_units(ph, unit_size), ss_y, d_dbl, dbl_stride, d_unit_ep, d_unit_xqd, d_unit_wiener), "sgr apply launch");
}
int svt_hip_lr_try_unit_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_dgd, int stride, void* d_dst, int dst_stride, int pw, int ph, int unit_size, int ss_y,
                            const void* d_dbl, int dbl_stride, const uint8_t* d_unit_ep, const int32_t* d_unit_xqd, const int16_t* d_unit_wiener, const void* d_src,
                            int src_stride, int unit, uint64_t* d_sse) {
    SVT_HIP_ENTER(c);
    if (!c || !d_dgd || !d_dst || !d_unit_ep || !d_unit_xqd || !d_src || !d_sse || !lr_plane_ok(pix_bytes, bd, pw, ph, unit_size, ss_y)) return bad_arg(c);
    const int ux = sgr_units(pw, unit_size), uy = sgr_units(ph, unit_size);
    if (unit < 0 || unit >= ux * uy) return bad_arg(c);
    // the unit's rectangle: foreach_rest_unit_in_tile (Common/Codec/EbRestoration.c:1369-1411) — the last unit of a row / column takes the remainder
    const int uj = unit % ux, ui = unit / ux, voff = 8 >> ss_y;
    const int x0 = uj * unit_size, w = uj == ux - 1 ? pw - x0 : unit_size;
    const int y0 = ui * unit_size, h = ui == uy - 1 ? ph - y0 : unit_size;
    const int v0 = y0 - voff > 0 ? y0 - voff : 0, v1 = (y0 + h < ph) ? y0 + h - voff : y0 + h;
    // tiles are 64 x 32 starting at (0, -voff): unit boundaries fall on tile boundaries
    const int tx0 = x0 / 64, tx1 = (x0 + w + 63) / 64, ty0 = (v0 + voff) / 32, ty1 = (v1 + voff + 31) / 32;
    if (int rc = launched(c, svt_hip_launch_sgr_apply_tiles(c->stream, pix_bytes, bd, d_dgd, stride, d_dst, dst_stride, pw, ph, unit_size, ux, uy, ss_y, d_dbl, dbl_stride, d_unit_ep,
                                                            d_unit_xqd, d_unit_wiener, tx0, ty0, tx1 - tx0, ty1 - ty0), "restoration unit launch"))
        return rc;
    HIPCHK(c, hipMemsetAsync(d_sse, 0, sizeof(uint64_t), c->stream));
    const uint8_t* a = (const uint8_t*)d_src + ((size_t)v0 * src_stride + x0) * pix_bytes;
    const uint8_t* b = (const uint8_t*)d_dst + ((size_t)v0 * dst_stride + x0) * pix_bytes;
    return launched(c, svt_hip_launch_plane_sse(c->stream, pix_bytes, a, src_stride, b, dst_stride, w, v1 - v0, d_sse), "restoration unit sse launch");
}
int svt_hip_lr_try_units_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_dgd, int stride, void* d_dst, int dst_stride, int pw, int ph, int unit_size, int ss_y,
                             const void* d_dbl, int dbl_stride, const uint8_t* d_unit_ep, const int32_t* d_unit_xqd, const int16_t* d_unit_wiener, const void* d_src,
                             int src_stride, const SvtHipBlkPair* d_rects, int n_rects, uint64_t* d_sse) {
    SVT_HIP_ENTER(c);
    if (!c || !d_src || !d_rects || !d_sse || n_rects < 0) return bad_arg(c);
    int rc = svt_hip_lr_apply_plane_dev(c, pix_bytes, bd, d_dgd, stride, d_dst, dst_stride, pw, ph, unit_size, ss_y, d_dbl, dbl_stride, d_unit_ep, d_unit_xqd, d_unit_wiener);
    if (rc != SVT_HIP_OK) return rc;
    return svt_hip_block_sse_batch_dev(c, pix_bytes, d_src, src_stride, d_dst, dst_stride, d_rects, n_rects, d_sse);
}

int svt_hip_wiener_walk_units_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_dgd, int stride, int pw, int ph, int unit_size, int ss_y, const void* d_dbl, int dbl_stride,
                                  const void* d_src, int src_stride, int16_t* d_unit_wiener, const uint8_t* d_active, int wiener_win, int64_t* d_err, uint32_t* d_probes) {
    SVT_HIP_ENTER(c);
    if (!c || !d_dgd || !d_src || !d_unit_wiener || !d_active || !d_err || (wiener_win != 7 && wiener_win != 5 && wiener_win != 3) || !lr_plane_ok(pix_bytes, bd, pw, ph, unit_size, ss_y))
        return bad_arg(c, "svt_hip_wiener_walk_units_dev: bad argument");
    const SvtHipWienerWalkPlane P = {d_dgd, stride, pw, ph, unit_size, ss_y, d_dbl, dbl_stride, d_src, src_stride, d_unit_wiener, d_active, wiener_win, d_err, d_probes};
    return launched(c, svt_hip_launch_wiener_walk_multi(c->stream, pix_bytes, bd, 1, &P), "wiener walk launch");
}

int svt_hip_wiener_walk_units_picture_dev(SvtHipCtx* c, int pix_bytes, int bd, int n_planes, const SvtHipWienerWalkPlane* planes) {
    SVT_HIP_ENTER(c);
    if (!c || !planes || n_planes < 1 || n_planes > 3) return bad_arg(c);
    for (int i = 0; i < n_planes; i++) {
        const SvtHipWienerWalkPlane& P = planes[i];
        if (!P.d_dgd || !P.d_src || !P.d_unit_wiener || !P.d_active || !P.d_err || (P.wiener_win != 7 && P.wiener_win != 5 && P.wiener_win != 3) || !lr_plane_ok(pix_bytes, bd, P.pw, P.ph, P.unit_size, P.ss_y))
            return bad_arg(c, "svt_hip_wiener_walk_units_picture_dev: bad plane");
    }
    return launched(c, svt_hip_launch_wiener_walk_multi(c->stream, pix_bytes, bd, n_planes, planes), "wiener walk launch");
}

int svt_hip_sgr_proj_error_plane_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_dgd, int stride, const void* d_src, int src_stride,
                                     int pw, int ph, int unit_size, int ss_y, uint32_t ep_mask, int ncand, const int32_t* d_xqd, int64_t* d_err) {
    SVT_HIP_ENTER(c);
    if (!c || !d_dgd || !d_src || !d_xqd || !d_err || ncand < 1 || ncand > SVT_HIP_SGR_MAX_CAND || !lr_plane_ok(pix_bytes, bd, pw, ph, unit_size, ss_y)) return bad_arg(c);
    const int ux = sgr_units(pw, unit_size), uy = sgr_units(ph, unit_size);
    HIPCHK(c, hipMemsetAsync(d_err, 0, sizeof(int64_t) * (size_t)ux * uy * 16 * ncand, c->stream));
    return launched(c, svt_hip_launch_sgr_proj_error(c->stream, pix_bytes, bd, d_dgd, stride, d_src, src_stride, pw, ph, unit_size, ux, uy, ss_y, ep_mask & 0xFFFFu,
                                                     ncand, d_xqd, d_err), "sgr proj error launch");
}

/* ---- search_selfguided_restoration (Encoder/Codec/EbRestorationPick.c:583-671) for every unit of a plane, entirely on the device ----
 * launch 1: sgr_search8_kernel<STORE>: the five projection sums of every (unit, set) + the int16 planes flt0 - u, flt1 - u, dat - src
 * then sgr_walk.hip: replay (one wave per (unit, set): solve, encode_xq, the walk on exact errors, best-first speculation) and evaluate launches alternate a
 * fixed number of times, a last launch writes the results and every unit's best set
 * No host synchronisation in between; the scratch (sums, arrival counters, difference planes) is the caller's. */
namespace {
struct SgrScratch { size_t stats, sums, d2, states, esc_cnt, sd, pairs, esc, total, dplane; int dstride, nu; };
// SVT_HIP_SGR_PACKED=1 (bit depth 8 only) runs the unit search on PACKED difference words (one 32-bit word per sample and set in `pairs`, no dat - src plane; sgr.hip
// STORE == 2, sgr_walk_packed_kernel).  A measured negative result, kept as the experiment it is (profiles/r06/sgr_packed_ab.txt): the form cuts the walk's memory traffic by a quarter (1.85 -> 1.41 GB per 4K frame) and
// raises its resident share from 38 % to 55-66 %, and the walk takes the same time -- its evaluation is bound by v_dot2 issue and by the one memory round trip per streamed chunk,
// not by bytes -- while the filter kernel pays 0.1 ms per 4K frame for the packing.  The default stays the 6-byte form.
// Read once per entry-point call (tests run both forms in one process) and handed down, so that the size that is checked and the form that is launched agree.
bool sgr_packed(int bd) {
    const char* env = getenv("SVT_HIP_SGR_PACKED");
    return bd == 8 && env && env[0] == '1';
}
SgrScratch sgr_scratch_layout(int pw, int ph, int unit_size, bool packed) {
    SgrScratch L;
    L.nu = sgr_units(pw, unit_size) * sgr_units(ph, unit_size);
    L.dstride = (pw + 63) & ~63;
    L.dplane = (size_t)L.dstride * (size_t)ph;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t o = 0;
    L.stats = o;    o = al(o + 128);   // diagnostics over the plane: [0] evaluation passes, [1] evaluated points, [2] unfinished walks, [24..30] phase clocks of the walks (sgr_walk.hip)
    L.sums = o;     o = al(o + sizeof(int64_t) * (size_t)L.nu * 16 * 5);
    L.d2 = o;       o = al(o + sizeof(int64_t) * (size_t)L.nu);   // sum (dat - src)^2 per unit
    L.states = o;   o = al(o + svt_hip_sgr_walk_state_bytes(L.nu));   // per (unit, set): cache of evaluated points, points wanted next, result
    L.esc_cnt = o;  o = al(o + sizeof(uint32_t) * (size_t)L.nu * 16);   // packed form: listed samples per (unit, set)
    L.sd = o;       o = al(o + sizeof(int16_t) * L.dplane);            // everything before this is cleared per call
    L.pairs = o;    o = al(o + sizeof(uint32_t) * L.dplane * 16);
    // packed form: the escape lists, 13 filter pairs x one 8-byte entry per sample (the worst case -- every sample of a binary test picture -- is what the lists are
    // sized for, so that there is no second code path for "too many"; coded pictures leave them empty and untouched); the 6-byte form ends here
    L.esc = o;
    L.total = packed ? al(o + sizeof(uint64_t) * L.dplane * 13) : o;
    return L;
}
// One plane of the unit search, for the _plane_dev and the _picture_dev form alike: the test of its arguments, then the store kernel's and the walk's view of the
// caller's scratch.  The entry point words the refusal (the two say "bad argument" and "bad plane").
enum SgrPlaneFault { SGR_PLANE_OK, SGR_PLANE_BAD, SGR_PLANE_SCRATCH };
SgrPlaneFault sgr_units_plane(int pix_bytes, int bd, bool packed, const SvtHipSgrUnitsPlaneDev& P, SgrScratch* layout, SvtHipSgrSearchStorePlane* sp, SvtHipSgrWalkPlane* wp) {
    const uint32_t ep_mask = P.ep_mask & 0xFFFFu;
    if (!P.d_dgd || !P.d_src || !P.d_xqd || !P.d_err || !P.d_scratch || !lr_plane_ok(pix_bytes, bd, P.pw, P.ph, P.unit_size, P.ss_y) || !ep_mask || ((uintptr_t)P.d_scratch & 15))
        return SGR_PLANE_BAD;
    const SgrScratch L = *layout = sgr_scratch_layout(P.pw, P.ph, P.unit_size, packed);
    if (P.scratch_bytes < L.total) return SGR_PLANE_SCRATCH;
    char* base = (char*)P.d_scratch;
    const int ux = sgr_units(P.pw, P.unit_size), uy = sgr_units(P.ph, P.unit_size);
    *sp = SvtHipSgrSearchStorePlane{P.d_dgd, P.d_src, (int64_t*)(base + L.sums), (uint32_t*)(base + L.pairs), (int16_t*)(base + L.sd), (int64_t*)(base + L.d2),
                                    packed ? base + L.esc : nullptr, (uint32_t*)(base + L.esc_cnt), L.dplane, P.stride, P.src_stride, P.pw, P.ph, P.unit_size, ux, uy, P.ss_y,
                                    L.dstride, ep_mask};
    *wp = SvtHipSgrWalkPlane{(const uint32_t*)(base + L.pairs), (const int16_t*)(base + L.sd), (const int64_t*)(base + L.sums), base + L.states, L.dplane, L.dstride,
                             P.pw, P.ph, P.unit_size, ux, uy, P.ss_y, ep_mask, P.d_xqd, P.d_err, P.d_best_ep, P.d_best_xqd, (uint32_t*)(base + L.stats),
                             packed ? base + L.esc : nullptr, (const uint32_t*)(base + L.esc_cnt)};
    return SGR_PLANE_OK;
}
}  // namespace

size_t svt_hip_sgr_search_units_scratch_bytes(int pw, int ph, int unit_size) {
    if (pw <= 0 || ph <= 0 || unit_size < 64 || (unit_size & 63)) return 0;
    return sgr_scratch_layout(pw, ph, unit_size, sgr_packed(8)).total;   // the packed experiment's lists count only while it is switched on
}

int svt_hip_sgr_search_units_plane_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_dgd, int stride, const void* d_src, int src_stride, int pw,
                                       int ph, int unit_size, int ss_y, uint32_t ep_mask, int32_t* d_xqd, int64_t* d_err, uint8_t* d_best_ep,
                                       int32_t* d_best_xqd, void* d_scratch, size_t scratch_bytes) {
    SVT_HIP_ENTER(c);
    const SvtHipSgrUnitsPlaneDev P = {d_dgd, stride, d_src, src_stride, pw, ph, unit_size, ss_y, ep_mask, d_xqd, d_err, d_best_ep, d_best_xqd, d_scratch, scratch_bytes};
    SgrScratch L;
    SvtHipSgrSearchStorePlane sp;
    SvtHipSgrWalkPlane wp;
    const SgrPlaneFault f = sgr_units_plane(pix_bytes, bd, sgr_packed(bd), P, &L, &sp, &wp);
    if (!c || f == SGR_PLANE_BAD) return bad_arg(c, "svt_hip_sgr_search_units_plane_dev: bad argument");
    if (f == SGR_PLANE_SCRATCH) return bad_arg(c, "svt_hip_sgr_search_units_plane_dev: scratch smaller than svt_hip_sgr_search_units_scratch_bytes()");
    char* base = (char*)d_scratch;
    HIPCHK(c, hipMemsetAsync(base, 0, L.sd, c->stream));   // statistics, sums, per-unit squared differences, the walk's arrival counters (one fill for all of them)
    if (int rc = launched(c, svt_hip_launch_sgr_search_store(c->stream, pix_bytes, bd, sp.dgd, sp.stride, sp.src, sp.src_stride, sp.pw, sp.ph, sp.unit_size, sp.units_x, sp.units_y,
                                                             sp.ss_y, sp.ep_mask, sp.sums, sp.pairs, sp.sd, sp.dstride, sp.dplane, sp.d2, sp.esc, sp.esc_cnt),
                          "sgr search (store) launch"))
        return rc;
    return launched(c, svt_hip_launch_sgr_walk_multi(c->stream, bd, 1, &wp), "sgr walk launch");
}

// All planes of a picture: ONE launch of the sums / difference-plane kernel, then ONE walk launch for every (plane, unit, set) — one tail each instead of three.
int svt_hip_sgr_search_units_picture_dev(SvtHipCtx* c, int pix_bytes, int bd, int n_planes, const SvtHipSgrUnitsPlaneDev* pl) {
    SVT_HIP_ENTER(c);
    if (!c || !pl || n_planes < 1 || n_planes > SVT_HIP_SGR_MAX_PLANES) return bad_arg(c);
    SvtHipSgrWalkPlane wp[SVT_HIP_SGR_MAX_PLANES];
    SvtHipSgrSearchStorePlane sp[SVT_HIP_SGR_MAX_PLANES];
    const bool packed = sgr_packed(bd);
    for (int i = 0; i < n_planes; i++) {
        SgrScratch L;
        const SgrPlaneFault f = sgr_units_plane(pix_bytes, bd, packed, pl[i], &L, &sp[i], &wp[i]);
        if (f == SGR_PLANE_BAD) return bad_arg(c, "svt_hip_sgr_search_units_picture_dev: bad plane");
        if (f == SGR_PLANE_SCRATCH) return bad_arg(c, "svt_hip_sgr_search_units_picture_dev: scratch smaller than svt_hip_sgr_search_units_scratch_bytes()");
        char* base = (char*)pl[i].d_scratch;
        HIPCHK(c, hipMemsetAsync(base, 0, L.sd, c->stream));   // ... and the walk's arrival counters
    }
    // one launch of the sums / difference-plane kernel for every plane (a chroma plane alone is one workgroup round: its launch lasts a workgroup's whole latency) ...
    if (int rc = launched(c, svt_hip_launch_sgr_search_store_multi(c->stream, pix_bytes, bd, n_planes, sp), "sgr search (store) launch")) return rc;
    // ... and one walk launch for every (plane, unit, set)
    return launched(c, svt_hip_launch_sgr_walk_multi(c->stream, bd, n_planes, wp), "sgr walk launch");
}

// HOST-output convenience forms: the library's own scratch, one synchronisation at the very end (to hand the results over).
int svt_hip_sgr_search_units_picture(SvtHipCtx* c, int pix_bytes, int bd, int n_planes, const SvtHipSgrSearchPlane* planes, int* rounds_out) {
    SVT_HIP_ENTER(c);
    if (!c || !planes || n_planes < 1 || n_planes > 3) return bad_arg(c);
    struct Off { size_t scratch, scratch_bytes, xqd, err, best; int nu; } off[3];
    size_t need = 0;
    const bool packed = sgr_packed(bd);
    for (int k = 0; k < n_planes; k++) {
        const SvtHipSgrSearchPlane& P = planes[k];
        if (!P.d_dgd || !P.d_src || !P.xqd_out || !P.err_out || !lr_plane_ok(pix_bytes, bd, P.pw, P.ph, P.unit_size, P.ss_y) || !(P.ep_mask & 0xFFFFu)) return bad_arg(c);
        const SgrScratch L = sgr_scratch_layout(P.pw, P.ph, P.unit_size, packed);
        auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
        off[k].nu = L.nu;
        off[k].scratch_bytes = L.total;
        off[k].scratch = need; need = al(need + L.total);
        off[k].xqd = need;     need = al(need + sizeof(int32_t) * (size_t)L.nu * 32);
        off[k].err = need;     need = al(need + sizeof(int64_t) * (size_t)L.nu * 16);
        off[k].best = need;    need = al(need + (size_t)L.nu);
    }
    if (int rc = grow_scratch(c, need)) return rc;
    char* dev = (char*)c->scratch;
    for (int k = 0; k < n_planes; k++) {
        const SvtHipSgrSearchPlane& P = planes[k];
        const int rc = svt_hip_sgr_search_units_plane_dev(c, pix_bytes, bd, P.d_dgd, P.stride, P.d_src, P.src_stride, P.pw, P.ph, P.unit_size, P.ss_y, P.ep_mask,
                                                          (int32_t*)(dev + off[k].xqd), (int64_t*)(dev + off[k].err), (uint8_t*)(dev + off[k].best), nullptr,
                                                          dev + off[k].scratch, off[k].scratch_bytes);
        if (rc != SVT_HIP_OK) return rc;
    }
    for (int k = 0; k < n_planes; k++) {
        const SvtHipSgrSearchPlane& P = planes[k];
        const size_t nu = (size_t)off[k].nu;
        std::vector<int32_t> xqd(nu * 32);
        std::vector<int64_t> err(nu * 16);
        HIPCHK(c, hipMemcpyAsync(xqd.data(), dev + off[k].xqd, sizeof(int32_t) * nu * 32, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(err.data(), dev + off[k].err, sizeof(int64_t) * nu * 16, hipMemcpyDeviceToHost, c->stream));
        if (P.best_ep) HIPCHK(c, hipMemcpyAsync(P.best_ep, dev + off[k].best, nu, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (size_t u = 0; u < nu; u++)
            for (int ep = 0; ep < 16; ep++) {
                if (!((P.ep_mask >> ep) & 1)) continue;   // sets outside the mask stay untouched
                if (err[u * 16 + ep] < 0) { c->err = "svt_hip_sgr_search_units: a walk did not finish within the pass budget"; return SVT_HIP_ERR_RUNTIME; }
                P.xqd_out[(u * 16 + ep) * 2] = xqd[(u * 16 + ep) * 2]; P.xqd_out[(u * 16 + ep) * 2 + 1] = xqd[(u * 16 + ep) * 2 + 1];
                P.err_out[u * 16 + ep] = err[u * 16 + ep];
            }
    }
    if (rounds_out) *rounds_out = 0;   // kept for source compatibility: there are no host rounds any more
    return SVT_HIP_OK;
}

int svt_hip_sgr_search_units_plane(SvtHipCtx* c, int pix_bytes, int bd, const void* d_dgd, int stride, const void* d_src, int src_stride, int pw,
                                   int ph, int unit_size, int ss_y, uint32_t ep_mask, int32_t* xqd_out, int64_t* err_out, uint8_t* best_ep, int* rounds_out) {
    SVT_HIP_ENTER(c);
    SvtHipSgrSearchPlane P = {d_dgd, stride, d_src, src_stride, pw, ph, unit_size, ss_y, ep_mask, xqd_out, err_out, best_ep};
    return svt_hip_sgr_search_units_picture(c, pix_bytes, bd, 1, &P, rounds_out);
}

int svt_hip_wiener_init_units_dev(SvtHipCtx* c, int win, int n_units, const int64_t* d_M, const int64_t* d_H, int16_t* d_unit_wiener, uint8_t* d_active, int8_t* d_status) {
    SVT_HIP_ENTER(c);
    if (!c || (win != 7 && win != 5 && win != 3) || n_units < 0 || (n_units && (!d_M || !d_H || !d_unit_wiener || !d_active || !d_status)))
        return bad_arg(c, "svt_hip_wiener_init_units_dev: bad argument");
    return launched(c, svt_hip_launch_wiener_init(c->stream, win, n_units, d_M, d_H, d_unit_wiener, d_active, d_status), "wiener init launch");
}

int svt_hip_wiener_stats_plane_dev(SvtHipCtx* c, int pix_bytes, int bd, int win, const void* d_dgd, int stride, const void* d_src, int src_stride,
                                   int pw, int ph, int unit_size, int ss_y, int64_t* d_M, int64_t* d_H) {
    SVT_HIP_ENTER(c);
    if (!c || !d_dgd || !d_src || !d_M || !d_H || (win != 7 && win != 5 && win != 3) || unit_size < 64 || (unit_size & 63) || unit_size > 256 ||
        (ss_y != 0 && ss_y != 1) || pw <= 0 || ph <= 0)
        return bad_arg(c);
    if (!fmt12_ok(pix_bytes, bd)) return bad_arg(c, "svt_hip_wiener_stats_plane_dev: bad sample format");
    if (pix_bytes == 2) {
        const int n_units = sgr_units(pw, unit_size) * sgr_units(ph, unit_size);
        const size_t need = svt_hip_wiener_stats16_scratch(win, pw, ph, n_units);
        if (int rc = grow_scratch(c, need)) return rc;
        return launched(c, svt_hip_launch_wiener_stats16(c->stream, win, bd, (const uint16_t*)d_dgd, stride, (const uint16_t*)d_src, src_stride, pw, ph, unit_size,
                                                         sgr_units(pw, unit_size), sgr_units(ph, unit_size), ss_y, d_M, d_H, (uint8_t*)c->scratch), "wiener stats (16-bit) launch");
    }
    return launched(c, svt_hip_launch_wiener_stats8(c->stream, win, (const uint8_t*)d_dgd, stride, (const uint8_t*)d_src, src_stride, pw, ph, unit_size,
                                                    sgr_units(pw, unit_size), sgr_units(ph, unit_size), ss_y, d_M, d_H), "wiener stats launch");
}

int svt_hip_tf_filter_frame_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* const d_src[3], const int src_stride[3], void* const d_dst[3],
                                const int dst_stride[3], int w, int h, int ss_x, int ss_y, int tf_chroma, const SvtHipTfRef* refs, int n_refs,
                                const double noise_levels[3], int decay_control, int min_frame_size, uint64_t* d_sse) {
    SVT_HIP_ENTER(c);
    if (!c || !d_src || !src_stride || !d_dst || !dst_stride || !refs || !noise_levels || !d_sse || !fmt_8to12_ok(pix_bytes, bd) || w <= 0 || h <= 0 ||
        (w & 63) || (h & 63) || n_refs < 1 || n_refs > SVT_HIP_TF_MAX_REFS || (ss_x != 0 && ss_x != 1) || (ss_y != 0 && ss_y != 1) || (ss_y == 1 && ss_x == 0) || decay_control <= 0)
        return bad_arg(c, "svt_hip_tf_filter_frame_dev: bad argument");
    for (int p = 0; p < (tf_chroma ? 3 : 1); p++) {
        if (!d_src[p] || !d_dst[p]) return bad_arg(c);
        for (int f = 0; f < n_refs; f++)
            if (refs[f].blocks && !refs[f].pred[p]) return bad_arg(c);
    }
    // the per-call scalars of EbTemporalFiltering.c:706 / :731-733, in the reference's own double arithmetic (host libm log1p)
    double den[3];
    for (int p = 0; p < 3; p++) {
        const double n_decay = (double)decay_control * (0.7 + log1p(noise_levels[p]));
        den[p] = 2 * n_decay * n_decay;
    }
    const double thr = min_frame_size * 0.1;
    const double dist_thr = thr > 1 ? thr : 1;
    if (int rc = launched(c, hipMemsetAsync(d_sse, 0, 2 * sizeof(uint64_t), c->stream), "tf sse memset")) return rc;
    return launched(c, svt_hip_launch_tf_filter(c->stream, pix_bytes, bd, d_src, src_stride, d_dst, dst_stride, w, h, ss_x, ss_y, tf_chroma, refs, n_refs, den, dist_thr, d_sse),
                    "tf filter launch");
}

int svt_hip_tf_estimate_noise_dev(SvtHipCtx* c, const void* d_src, int pix_bytes, int bd, int width, int height, int stride, int64_t* d_out) {
    SVT_HIP_ENTER(c);
    if (!c || !d_src || !d_out || !fmt_8to12_ok(pix_bytes, bd) || width <= 0 || height <= 0 || stride < width) return bad_arg(c);
    if (int rc = launched(c, hipMemsetAsync(d_out, 0, 2 * sizeof(int64_t), c->stream), "tf noise memset")) return rc;
    return launched(c, svt_hip_launch_tf_noise(c->stream, d_src, pix_bytes, bd, width, height, stride, (uint64_t*)d_out), "tf noise launch");
}

int svt_hip_tf_subpel_frame_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* const d_src[3], const int src_stride[3], const void* const d_ref[3],
                                const int ref_stride[3], void* const d_pred[3], const int pred_stride[3], int mi_cols, int mi_rows, uint64_t th16, int tf_hp,
                                int tf_chroma, const SvtHipTfSubpelBlk* d_jobs, int n_jobs, SvtHipTfBlk64* d_blocks) {
    SVT_HIP_ENTER(c);
    if (!c || !d_src || !src_stride || !d_ref || !ref_stride || !d_pred || !pred_stride || !d_jobs || !d_blocks || n_jobs < 0 || mi_cols <= 0 || mi_rows <= 0 ||
        !fmt_ok(pix_bytes, bd))
        return bad_arg(c, "svt_hip_tf_subpel_frame_dev: bad argument");
    for (int p = 0; p < (tf_chroma ? 3 : 1); p++)
        if (!d_src[p] || !d_ref[p] || !d_pred[p]) return bad_arg(c);
    return launched(c, svt_hip_launch_tf_subpel(c->stream, pix_bytes, bd, d_src, src_stride, d_ref, ref_stride, d_pred, pred_stride, mi_cols, mi_rows, th16, tf_hp != 0,
                                                tf_chroma != 0, d_jobs, n_jobs, d_blocks), "tf sub-pel launch");
}

int svt_hip_compound_predict_batch_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_ref0, int ref0_stride, const void* d_ref1, int ref1_stride,
                                       void* d_dst, int dst_stride, uint8_t* d_masks, const SvtHipCompBlk* d_blks, int nblk) {
    SVT_HIP_ENTER(c);
    if (!c || nblk < 0 || !fmt12_ok(pix_bytes, bd))
        return bad_arg(c, "svt_hip_compound_predict_batch_dev: bad argument");
    if (nblk == 0) return SVT_HIP_OK;
    if (!d_ref0 || !d_ref1 || !d_dst || !d_blks) return bad_arg(c);
    return launched(c, svt_hip_launch_compound_predict(c->stream, pix_bytes, bd, d_ref0, ref0_stride, d_ref1, ref1_stride, d_dst, dst_stride, d_masks, d_blks, nblk),
                    "compound predict launch");
}

int svt_hip_obmc_cost_batch_dev(SvtHipCtx* c, const uint8_t* d_pre, int pre_stride, const int32_t* d_wsrc, const int32_t* d_mask, const SvtHipObmcBlk* d_blks,
                                int nblk, uint32_t* d_out) {
    SVT_HIP_ENTER(c);
    if (!c || nblk < 0) return bad_arg(c);
    if (nblk == 0) return SVT_HIP_OK;
    if (!d_pre || !d_wsrc || !d_mask || !d_blks || !d_out) return bad_arg(c);
    return launched(c, svt_hip_launch_obmc_cost(c->stream, d_pre, pre_stride, d_wsrc, d_mask, d_blks, nblk, d_out), "obmc cost launch");
}

int svt_hip_warp_predict_batch_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_ref, int width, int height, int stride, void* d_dst, int dst_stride,
                                   int ss_x, int ss_y, const SvtHipWarpBlk* d_blks, int nblk) {
    SVT_HIP_ENTER(c);
    if (!c || nblk < 0 || !fmt12_ok(pix_bytes, bd) ||
        (ss_x != 0 && ss_x != 1) || (ss_y != 0 && ss_y != 1))
        return bad_arg(c, "svt_hip_warp_predict_batch_dev: bad argument");
    if (nblk == 0) return SVT_HIP_OK;
    if (!d_ref || !d_dst || !d_blks || width <= 0 || height <= 0) return bad_arg(c);
    return launched(c, svt_hip_launch_warp_predict(c->stream, pix_bytes, bd, d_ref, width, height, stride, d_dst, dst_stride, ss_x, ss_y, d_blks, nblk), "warp predict launch");
}
int svt_hip_warp_compound_batch_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_ref, int width, int height, int stride, void* d_dst, int dst_stride,
                                    int ss_x, int ss_y, uint16_t* d_convbuf, const SvtHipWarpCompBlk* d_blks, int nblk) {
    SVT_HIP_ENTER(c);
    if (!c || nblk < 0 || !fmt12_ok(pix_bytes, bd) ||
        (ss_x != 0 && ss_x != 1) || (ss_y != 0 && ss_y != 1))
        return bad_arg(c, "svt_hip_warp_compound_batch_dev: bad argument");
    if (nblk == 0) return SVT_HIP_OK;
    if (!d_ref || !d_convbuf || !d_blks || width <= 0 || height <= 0) return bad_arg(c);   // d_dst may be NULL when no block averages
    return launched(c, svt_hip_launch_warp_compound(c->stream, pix_bytes, bd, d_ref, width, height, stride, d_dst, dst_stride, ss_x, ss_y, d_convbuf, d_blks, nblk),
                    "warp compound launch");
}

int svt_hip_blend_a64_batch_dev(SvtHipCtx* c, int pix_bytes, const void* d_src0, int src0_stride, const void* d_src1, int src1_stride, void* d_dst, int dst_stride,
                                const uint8_t* d_masks, const SvtHipBlendBlk* d_blks, int nblk) {
    SVT_HIP_ENTER(c);
    if (!c || nblk < 0 || !pix_ok(pix_bytes)) return bad_arg(c);
    if (nblk == 0) return SVT_HIP_OK;
    if (!d_src0 || !d_src1 || !d_dst || !d_masks || !d_blks) return bad_arg(c);
    return launched(c, svt_hip_launch_blend_a64(c->stream, pix_bytes, d_src0, src0_stride, d_src1, src1_stride, d_dst, dst_stride, d_masks, d_blks, nblk), "blend_a64 launch");
}

int svt_hip_picture_format_dev(SvtHipCtx* c, int mode, const void* d_in0, int in0_stride, const void* d_in1, int in1_stride, void* d_out0, int out0_stride,
                               void* d_out1, int out1_stride, int w, int h) {
    SVT_HIP_ENTER(c);
    const bool two_in = mode == 0 || mode == 1 || mode == 6;
    if (!c || mode < 0 || mode > 6 || w < 0 || h < 0 || ((mode == 1 || mode == 5) && (w & 3))) return bad_arg(c, "svt_hip_picture_format_dev: bad argument");
    if (w == 0 || h == 0) return SVT_HIP_OK;
    if (!d_in0 || !d_out0 || (two_in && !d_in1)) return bad_arg(c);
    return launched(c, svt_hip_launch_picture_format(c->stream, mode, d_in0, in0_stride, d_in1, in1_stride, d_out0, out0_stride, d_out1, out1_stride, w, h),
                    "picture format launch");
}

int svt_hip_generate_padding_dev(SvtHipCtx* c, void* d_plane, int pix_bytes, int stride, int w, int h, int pad_w, int pad_h) {
    SVT_HIP_ENTER(c);
    if (!c || !pix_ok(pix_bytes) || w < 0 || h < 0 || pad_w < 0 || pad_h < 0) return bad_arg(c);
    if (w == 0 || h == 0 || (pad_w == 0 && pad_h == 0)) return SVT_HIP_OK;
    if (!d_plane || stride < w + pad_w) return bad_arg(c);
    return launched(c, svt_hip_launch_generate_padding(c->stream, d_plane, pix_bytes, stride, w, h, pad_w, pad_h), "generate padding launch");
}

/* ------------------------------------------------------------------ super-resolution (resize.hip; the host arithmetic is resize_plan.h) */
int svt_hip_superres_scaled_dim(int dim, int denom) { return dim < 1 || dim > 65535 || denom < 8 || denom > 16 ? 0 : svt_superres_scaled_dim(dim, denom); }

int svt_hip_superres_upscale_params(int in_w, int out_w, int32_t* x_step_qn, int32_t* x0_qn) {
    if (in_w < 1 || out_w < in_w || out_w > SVT_RS_MAX_DIM || !x_step_qn || !x0_qn) return SVT_HIP_ERR_BAD_ARG;
    *x_step_qn = svt_superres_step_qn(in_w, out_w);
    *x0_qn = svt_superres_x0_qn(in_w, out_w, *x_step_qn);
    return SVT_HIP_OK;
}

static bool upscale_planes_ok(const SvtHipUpscalePlane* p, int n) {
    if (!p || n < 1 || n > 3) return false;
    for (int i = 0; i < n; i++)
        if (!svt_upscale_plane_ok(p[i])) return false;
    return true;
}
static bool resize_planes_ok(const SvtHipResizePlane* p, int n) {
    if (!p || n < 1 || n > 3) return false;
    for (int i = 0; i < n; i++)
        if (!svt_resize_plane_ok(p[i])) return false;
    return true;
}

int svt_hip_superres_upscale_planes_dev(SvtHipCtx* c, int pix_bytes, int bd, const SvtHipUpscalePlane* planes, int n_planes) {
    SVT_HIP_ENTER(c);
    if (!c || !fmt_8to12_ok(pix_bytes, bd) || !upscale_planes_ok(planes, n_planes))
        return bad_arg(c, "svt_hip_superres_upscale_planes_dev: bad argument (1 <= n_planes <= 3, 1 <= in_w <= out_w <= 16384, 1 <= rows <= 16384, stride >= width, d_src != d_dst)");
    return launched(c, svt_hip_launch_superres_upscale(c->stream, pix_bytes, bd, planes, n_planes), "super-resolution upscale launch");
}

size_t svt_hip_resize_scratch_bytes(int pix_bytes, const SvtHipResizePlane* planes, int n_planes) {
    if (!pix_ok(pix_bytes) || !resize_planes_ok(planes, n_planes)) return 0;
    return svt_hip_resize_scratch_layout_bytes(pix_bytes, planes, n_planes);
}

int svt_hip_resize_planes_dev(SvtHipCtx* c, int pix_bytes, int bd, const SvtHipResizePlane* planes, int n_planes, void* d_scratch, size_t scratch_bytes) {
    SVT_HIP_ENTER(c);
    if (!c || !fmt_8to12_ok(pix_bytes, bd) || !resize_planes_ok(planes, n_planes))
        return bad_arg(c, "svt_hip_resize_planes_dev: bad argument (1 <= n_planes <= 3, every size 1 .. 16384, stride >= width, d_src != d_dst)");
    const size_t need = svt_hip_resize_scratch_layout_bytes(pix_bytes, planes, n_planes);
    if (need && (!d_scratch || scratch_bytes < need)) return bad_arg(c, "svt_hip_resize_planes_dev: d_scratch holds less than svt_hip_resize_scratch_bytes");
    return launched(c, svt_hip_launch_resize_planes(c->stream, pix_bytes, bd, planes, n_planes, d_scratch), "resize launch");
}


/* ------------------------------------------------------------------ prediction from a reference of another size (scaled_pred.hip; the arithmetic is scaled_pred.h) */
int svt_hip_scale_factors(int other_w, int other_h, int this_w, int this_h, SvtHipScaleFactors* out) {
    if (!out) return SVT_HIP_ERR_BAD_ARG;
    return sp_scale_factors(other_w, other_h, this_w, this_h, out) ? SVT_HIP_OK : SVT_HIP_ERR_BAD_ARG;
}

void svt_hip_scaled_block_params(const SvtHipScaleFactors* sf, int pre_x, int pre_y, int mv_row, int mv_col, int ss_x, int ss_y, int frame_w, int frame_h, int32_t* pos_x,
                                 int32_t* pos_y, int32_t* subpel_x, int32_t* subpel_y, int32_t* xs, int32_t* ys) {
    sp_block_params(*sf, pre_x, pre_y, mv_row, mv_col, ss_x & 1, ss_y & 1, frame_w, frame_h, pos_x, pos_y, subpel_x, subpel_y, xs, ys);
}

int svt_hip_scaled_jobs_dev(SvtHipCtx* c, const SvtHipScaleFactors* sf0, const SvtHipScaleFactors* sf1, const int frame_w[2], const int frame_h[2],
                            const SvtHipScaledRec* d_recs, SvtHipScaledBlk* d_jobs, int n) {
    SVT_HIP_ENTER(c);
    if (!c || n < 0 || !sf0 || !frame_w || !frame_h || !sp_scale_factors_ok(*sf0) || (sf1 && !sp_scale_factors_ok(*sf1)) || frame_w[0] < 1 || frame_w[0] > 65535 ||
        frame_h[0] < 1 || frame_h[0] > 65535 || (sf1 && (frame_w[1] < 1 || frame_w[1] > 65535 || frame_h[1] < 1 || frame_h[1] > 65535)))
        return bad_arg(c, "svt_hip_scaled_jobs_dev: bad argument (n >= 0, valid scale factors, every frame size 1 .. 65535)");
    if (n == 0) return SVT_HIP_OK;
    if (!d_recs || !d_jobs) return bad_arg(c, "svt_hip_scaled_jobs_dev: d_recs or d_jobs is NULL");
    const int fw[2] = {frame_w[0], sf1 ? frame_w[1] : frame_w[0]}, fh[2] = {frame_h[0], sf1 ? frame_h[1] : frame_h[0]};
    return launched(c, svt_hip_launch_scaled_jobs(c->stream, sf0, sf1 ? sf1 : sf0, fw, fh, d_recs, d_jobs, n), "scaled jobs launch");
}

int svt_hip_scaled_predict_batch_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_ref0, int ref0_stride, const void* d_ref1, int ref1_stride, void* d_dst,
                                     int dst_stride, const SvtHipScaledBlk* d_jobs, int n) {
    SVT_HIP_ENTER(c);
    if (!c || n < 0 || !fmt12_ok(pix_bytes, bd))
        return bad_arg(c, "svt_hip_scaled_predict_batch_dev: bad argument (n >= 0; samples (1, 8), (2, 8), (2, 10) or (2, 12))");
    if (n == 0) return SVT_HIP_OK;
    if (!d_ref0 || !d_dst || !d_jobs) return bad_arg(c, "svt_hip_scaled_predict_batch_dev: d_ref0, d_dst or d_jobs is NULL");   // d_ref1 may be: no job is compound
    return launched(c, svt_hip_launch_scaled_predict(c->stream, pix_bytes, bd, d_ref0, ref0_stride, d_ref1, ref1_stride, d_dst, dst_stride, d_jobs, n),
                    "scaled predict launch");
}


/* ------------------------------------------------------------------ per-call forms (percall.hip, cdef.hip, deblock.hip) */
int svt_hip_quantize_batch_dev(SvtHipCtx* c, const int32_t* d_coeff, int n_coeffs, int nblk, const SvtHipQuantParams* qp, const int16_t* d_iscan,
                               int32_t* d_qcoeff, int32_t* d_dqcoeff, uint16_t* d_eob) {
    SVT_HIP_ENTER(c);
    if (!c || !d_coeff || !qp || !d_iscan || !d_qcoeff || !d_dqcoeff || !d_eob || n_coeffs <= 0 || n_coeffs > 4096 || nblk < 0 || qp->variant < 0 || qp->variant > 3 ||
        qp->log_scale < 0 || qp->log_scale > 2)
        return bad_arg(c);
    return launched(c, svt_hip_launch_quantize_blocks(c->stream, d_coeff, n_coeffs, nblk, qp, d_iscan, d_qcoeff, d_dqcoeff, d_eob), "quantize launch");
}
int svt_hip_residual_dev(SvtHipCtx* c, int pix_bytes, const void* d_src, int src_stride, const void* d_pred, int pred_stride, int16_t* d_residual,
                         int residual_stride, int w, int h) {
    SVT_HIP_ENTER(c);
    if (!c || !pix_ok(pix_bytes) || w < 0 || h < 0) return bad_arg(c);
    if (w == 0 || h == 0) return SVT_HIP_OK;
    if (!d_src || !d_pred || !d_residual) return bad_arg(c);
    return launched(c, svt_hip_launch_residual(c->stream, pix_bytes, d_src, src_stride, d_pred, pred_stride, d_residual, residual_stride, w, h), "residual launch");
}
int svt_hip_ext_all_sad_8x8_16x16_batch_dev(SvtHipCtx* c, const uint8_t* d_src, int src_stride, const uint8_t* d_ref, int ref_stride,
                                            const SvtHipExtSadJob* d_jobs, int n, uint32_t* d_state) {
    SVT_HIP_ENTER(c);
    if (!c || !d_src || !d_ref || !d_jobs || !d_state || n < 0) return bad_arg(c);
    return launched(c, svt_hip_launch_ext_all_sad(c->stream, d_src, src_stride, d_ref, ref_stride, d_jobs, n, d_state), "ext all sad launch");
}
int svt_hip_ext_eight_sad_32x32_64x64_batch_dev(SvtHipCtx* c, const uint32_t* d_mv, int n, uint32_t* d_state) {
    SVT_HIP_ENTER(c);
    if (!c || !d_mv || !d_state || n < 0) return bad_arg(c);
    return launched(c, svt_hip_launch_ext_eight_sad_32_64(c->stream, d_mv, n, d_state), "ext eight sad launch");
}
int svt_hip_interm_var_four8x8_batch_dev(SvtHipCtx* c, const uint8_t* d_plane, int stride, const int32_t* d_offs, int n, uint64_t* d_mean, uint64_t* d_mean_sq) {
    SVT_HIP_ENTER(c);
    if (!c || !d_plane || !d_offs || !d_mean || !d_mean_sq || n < 0) return bad_arg(c);
    return launched(c, svt_hip_launch_interm_var(c->stream, d_plane, stride, d_offs, n, d_mean, d_mean_sq), "interm var launch");
}
int svt_hip_handle_transform64_batch_dev(SvtHipCtx* c, int tx_size, int32_t* d_coeff, int nblk, uint64_t* d_energy) {
    SVT_HIP_ENTER(c);
    if (!c || !d_coeff || !d_energy || nblk < 0 || (tx_size != 4 && tx_size != 11 && tx_size != 12 && tx_size != 17 && tx_size != 18)) return bad_arg(c);
    return launched(c, svt_hip_launch_handle_transform64(c->stream, tx_size, d_coeff, nblk, d_energy), "handle transform64 launch");
}
int svt_hip_upsampled_pred_batch_dev(SvtHipCtx* c, const uint8_t* d_ref, int ref_stride, uint8_t* d_dst, const SvtHipUpsampledBlk* d_blks, int n) {
    SVT_HIP_ENTER(c);
    if (!c || !d_ref || !d_dst || !d_blks || n < 0) return bad_arg(c);
    return launched(c, svt_hip_launch_upsampled_pred(c->stream, d_ref, ref_stride, d_dst, d_blks, n), "upsampled pred launch");
}
int svt_hip_handle_transform64_n2n4_batch_dev(SvtHipCtx* c, int tx_size, int32_t* d_coeff, int nblk) {
    SVT_HIP_ENTER(c);
    if (!c || !d_coeff || nblk < 0 || (tx_size != 4 && tx_size != 11 && tx_size != 12 && tx_size != 17 && tx_size != 18)) return bad_arg(c);
    if (tx_size == 11 || tx_size == 17) return SVT_HIP_OK;   // 32x64 / 16x64: the reference's functions do nothing
    const int rows = tx_size == 18 ? 16 : 32;
    return launched(c, svt_hip_launch_repack64(c->stream, d_coeff, rows, 64 * (tx_size == 4 ? 64 : rows), nblk), "handle transform64 N2 / N4 launch");
}
int svt_hip_diffwtd_mask_dev(SvtHipCtx* c, int elem_bytes, uint8_t* d_mask, const void* d_src0, int src0_stride, const void* d_src1, int src1_stride, int w, int h, int inverse,
                             int round, int shift) {
    SVT_HIP_ENTER(c);
    if (!c || !d_mask || !d_src0 || !d_src1 || w < 1 || h < 1 || !pix_ok(elem_bytes) || round < 0 || round > 15 || shift < 0 || shift > 8) return bad_arg(c);
    return launched(c, svt_hip_launch_diffwtd_mask(c->stream, elem_bytes, d_mask, d_src0, src0_stride, d_src1, src1_stride, w, h, inverse, round, shift), "diffwtd mask launch");
}
int svt_hip_blend_a64_d16_dev(SvtHipCtx* c, int pix_bytes, int bd, void* d_dst, int dst_stride, const uint16_t* d_src0, int src0_stride, const uint16_t* d_src1, int src1_stride,
                              const uint8_t* d_mask, int mask_stride, int w, int h, int subw, int subh, int round_0, int round_1) {
    SVT_HIP_ENTER(c);
    if (!c || !d_dst || !d_src0 || !d_src1 || !d_mask || w < 1 || h < 1 || !fmt_8to12_ok(pix_bytes, bd) || round_0 < 3 || round_0 > 5 ||
        round_1 < 1 || 14 - round_0 - round_1 < 0)
        return bad_arg(c);
    return launched(c, svt_hip_launch_blend_d16(c->stream, pix_bytes, bd, d_dst, dst_stride, d_src0, src0_stride, d_src1, src1_stride, d_mask, mask_stride, w, h,
                                                subw != 0, subh != 0, round_0, round_1), "blend a64 d16 launch");
}
int svt_hip_jnt_convolve_dev(SvtHipCtx* c, int pix_bytes, int bd, int variant, const void* d_src, int src_stride, void* d_dst, int dst_stride, uint16_t* d_convbuf,
                             int convbuf_stride, const int16_t* d_taps, int w, int h, int round_0, int round_1, int do_average, int use_jnt_comp_avg, int fwd_offset,
                             int bck_offset) {
    SVT_HIP_ENTER(c);
    if (!c || !d_src || !d_convbuf || !d_taps || (do_average && !d_dst) || w < 1 || h < 1 || variant < 0 || variant > 3 ||
        !fmt_8to12_ok(pix_bytes, bd) || round_0 < 3 || round_0 > 5 || round_1 < 1 || 14 - round_0 - round_1 < 0)
        return bad_arg(c);
    return launched(c, svt_hip_launch_jnt_convolve(c->stream, pix_bytes, bd, variant, d_src, src_stride, d_dst, dst_stride, d_convbuf, convbuf_stride, d_taps, w, h,
                                                   round_0, round_1, do_average, use_jnt_comp_avg, fwd_offset, bck_offset), "jnt convolve launch");
}
int svt_hip_block_mean_batch_dev(SvtHipCtx* c, const uint8_t* d_plane, int stride, const int32_t* d_offs, int n, int mode, int w, int h, uint64_t* d_out) {
    SVT_HIP_ENTER(c);
    if (!c || !d_plane || !d_offs || !d_out || n < 0 || (mode != 0 && mode != 1) || (mode == 0 && (w < 1 || h < 1))) return bad_arg(c);
    return launched(c, svt_hip_launch_block_mean(c->stream, d_plane, stride, d_offs, n, mode, w, h, d_out), "block mean launch");
}
int svt_hip_ext_sad_16x16_batch_dev(SvtHipCtx* c, const uint8_t* d_src, int src_stride, const uint8_t* d_ref, int ref_stride, const SvtHipExtSadJob* d_jobs, int n,
                                    uint32_t* d_state) {
    SVT_HIP_ENTER(c);
    if (!c || !d_src || !d_ref || !d_jobs || !d_state || n < 0) return bad_arg(c);
    return launched(c, svt_hip_launch_ext_sad_16(c->stream, d_src, src_stride, d_ref, ref_stride, d_jobs, n, d_state), "ext sad 16x16 launch");
}
int svt_hip_ext_sad_32x32_64x64_batch_dev(SvtHipCtx* c, uint32_t* d_state, const uint32_t* d_mv, int n) {
    SVT_HIP_ENTER(c);
    if (!c || !d_state || !d_mv || n < 0) return bad_arg(c);
    return launched(c, svt_hip_launch_ext_sad_32_64(c->stream, d_state, d_mv, n), "ext sad 32x32 / 64x64 launch");
}
int svt_hip_cdef_dist_dev(SvtHipCtx* c, int pix_bytes, const void* d_dst, int dstride, const void* d_src, const uint8_t* d_list, int n, int bw_log2, int bh_log2,
                          int coeff_shift, int pli, uint64_t* d_out) {
    SVT_HIP_ENTER(c);
    if (!c || !d_dst || !d_src || !d_list || !d_out || n < 0 || !pix_ok(pix_bytes) || (bw_log2 != 2 && bw_log2 != 3) || (bh_log2 != 2 && bh_log2 != 3) ||
        coeff_shift < 0 || coeff_shift > 4)
        return bad_arg(c);
    return launched(c, svt_hip_launch_cdef_dist(c->stream, pix_bytes, d_dst, dstride, d_src, d_list, n, bw_log2, bh_log2, coeff_shift, pli, d_out), "cdef dist launch");
}
/* ---------------------------------------------------------------- CDEF strength decision (cdef_select.hip) */
int svt_hip_cdef_search_one_dual_dev(SvtHipCtx* c, const uint64_t* d_mse0, const uint64_t* d_mse1, int sb_count, int* d_lev0, int* d_lev1, int nb_strengths, int start_gi,
                                     int end_gi, uint64_t* d_work) {
    SVT_HIP_ENTER(c);
    if (!c || !d_mse0 || !d_mse1 || !d_lev0 || !d_lev1 || !d_work || sb_count < 0 || nb_strengths < 0 || nb_strengths > 7 || start_gi < 0 || end_gi > 64 || start_gi > end_gi)
        return bad_arg(c);
    return launched(c, svt_hip_launch_search_one_dual(c->stream, d_mse0, d_mse1, sb_count, d_lev0, d_lev1, nb_strengths, start_gi, end_gi, d_work + 1 + 4096, d_work + 1,
                                                      d_work), "search one dual launch");
}
int svt_hip_cdef_joint_strength_search_dev(SvtHipCtx* c, const uint64_t* d_mse0, const uint64_t* d_mse1, int sb_count, int* d_lev0, int* d_lev1, int nb_strengths, int start_gi,
                                           int end_gi, uint64_t* d_work) {
    SVT_HIP_ENTER(c);
    if (!c || !d_mse0 || !d_mse1 || !d_lev0 || !d_lev1 || !d_work || sb_count < 0 || nb_strengths < 1 || nb_strengths > 8 || start_gi < 0 || end_gi > 64 || start_gi > end_gi)
        return bad_arg(c);
    return launched(c, svt_hip_launch_joint_strength_search(c->stream, d_mse0, d_mse1, sb_count, d_lev0, d_lev1, nb_strengths, start_gi, end_gi, d_work + 1 + 4096,
                                                            d_work + 1, d_work), "joint strength search launch");
}
int svt_hip_set_cdef_select_form(SvtHipCtx* c, int form) {
    if (!c || form < -1 || form > 1) return bad_arg(c);
    c->select_form = form;
    return SVT_HIP_OK;
}
int svt_hip_cdef_strength_select_dev(SvtHipCtx* c, const uint64_t* d_mse0, const uint64_t* d_mse1, int sb_count, int start_gi, int end_gi, void* d_state, size_t state_bytes) {
    SVT_HIP_ENTER(c);
    if (!c || !d_mse0 || !d_mse1 || !d_state || sb_count < 0 || start_gi < 0 || end_gi > 64 || start_gi > end_gi || state_bytes < svt_hip_joint_state_bytes())
        return bad_arg(c);
    return svt_hip_cdef_strength_select_multi_dev(c, 1, &d_mse0, &d_mse1, sb_count, start_gi, end_gi, &d_state, state_bytes);
}
int svt_hip_cdef_strength_select_multi_dev(SvtHipCtx* c, int n_pictures, const uint64_t* const* d_mse0, const uint64_t* const* d_mse1, int sb_count, int start_gi, int end_gi,
                                           void* const* d_states, size_t state_bytes) {
    SVT_HIP_ENTER(c);
    if (!c || n_pictures < 0 || !d_mse0 || !d_mse1 || !d_states || sb_count < 0 || start_gi < 0 || end_gi > 64 || start_gi > end_gi || state_bytes < svt_hip_joint_state_bytes())
        return bad_arg(c);
    for (int i = 0; i < n_pictures; i++)
        if (!d_mse0[i] || !d_mse1[i] || !d_states[i]) return bad_arg(c);
    hipStream_t sel = c->device < 64 ? g_sel_stream[c->device] : nullptr;
    const int resident = svt_hip_strength_select_is_resident(c->select_form, sb_count) && sel;
    if (!resident)
        return launched(c, svt_hip_launch_strength_select_multi(c->stream, n_pictures, d_mse0, d_mse1, sb_count, start_gi, end_gi, d_states, 0), "strength select (multi) launch");
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    unsigned long long     cap_id = 0;
    if (hipStreamGetCaptureInfo(c->stream, &cap, &cap_id) != hipSuccess) cap = hipStreamCaptureStatusNone;
    if (cap == hipStreamCaptureStatusActive) {
        std::lock_guard<std::mutex> lk(g_sel_mutex);
        const int d = c->device;
        if (g_sel_cap_event[d] && g_sel_cap_id[d] == cap_id) HIPCHK(c, hipStreamWaitEvent(c->stream, g_sel_cap_event[d], 0));
        if (int rc = launched(c, svt_hip_launch_strength_select_multi(c->stream, n_pictures, d_mse0, d_mse1, sb_count, start_gi, end_gi, d_states, 1), "strength select (multi) launch"))
            return rc;
        hipEvent_t ev = nullptr;
        HIPCHK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIPCHK(c, hipEventRecord(ev, c->stream));
        g_sel_cap_event[d] = ev; g_sel_cap_id[d] = cap_id;
        return SVT_HIP_OK;
    }
    HIPCHK(c, hipEventRecord(c->ev_sel_in, c->stream));
    {
        std::lock_guard<std::mutex> lk(g_sel_mutex);   // wait / launches / record of one call stay together on the shared stream
        HIPCHK(c, hipStreamWaitEvent(sel, c->ev_sel_in, 0));
        if (int rc = launched(c, svt_hip_launch_strength_select_multi(sel, n_pictures, d_mse0, d_mse1, sb_count, start_gi, end_gi, d_states, 1), "strength select (multi) launch"))
            return rc;
        HIPCHK(c, hipEventRecord(c->ev_sel_out, sel));
    }
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_sel_out, 0));
    return SVT_HIP_OK;
}
int svt_hip_cdef_finish_dev(SvtHipCtx* c, const uint64_t* d_mse0, const uint64_t* d_mse1, int sb_count, const void* d_state, uint64_t lambda, const int32_t* d_sb_fb,
                            SvtHipCdefFinish* d_out, int32_t* d_sel_gi, uint8_t* d_fb_y, uint8_t* d_fb_uv) {
    SVT_HIP_ENTER(c);
    if (!c || !d_mse0 || !d_mse1 || !d_state || !d_out || sb_count < 0) return bad_arg(c);
    return launched(c, svt_hip_launch_cdef_finish(c->stream, d_mse0, d_mse1, sb_count, d_state, lambda, d_sb_fb, d_out, d_sel_gi, d_fb_y, d_fb_uv), "cdef finish launch");
}
/* ------------------------------------------------------- per-call forms, continued (percall.hip, cdef.hip, deblock.hip) */
int svt_hip_sgr_flt_proj_dev(SvtHipCtx* c, int pix_bytes, const void* d_src, int src_stride, const void* d_dat, int dat_stride, const int32_t* d_flt0, int flt0_stride,
                             const int32_t* d_flt1, int flt1_stride, int w, int h, int r0, int r1, int mode, const int32_t* xq, int64_t* d_acc, int32_t* d_xq) {
    SVT_HIP_ENTER(c);
    if (!c || !d_src || !d_dat || !d_acc || w < 1 || h < 1 || !pix_ok(pix_bytes) || (mode != 0 && mode != 1) || (r0 > 0 && !d_flt0) || (r1 > 0 && !d_flt1) ||
        (mode == 0 && !d_xq) || (mode == 1 && !xq))
        return bad_arg(c);
    if (int rc = launched(c, hipMemsetAsync(d_acc, 0, 5 * sizeof(int64_t), c->stream), "sgr flt proj clear")) return rc;
    return launched(c, svt_hip_launch_sgr_flt_proj(c->stream, pix_bytes, d_src, src_stride, d_dat, dat_stride, d_flt0, flt0_stride, d_flt1, flt1_stride, w, h, r0, r1, mode,
                                                   mode ? xq[0] : 0, mode ? xq[1] : 0, (long long*)d_acc, d_xq), "sgr flt proj launch");
}
int svt_hip_convolve8_dev(SvtHipCtx* c, int vert, const uint8_t* d_src, int src_stride, uint8_t* d_dst, int dst_stride, const int16_t* d_filters, int q0, int step_q4, int w,
                          int h) {
    SVT_HIP_ENTER(c);
    if (!c || !d_src || !d_dst || !d_filters || w < 1 || h < 1 || q0 < 0 || q0 > 15 || step_q4 < 1 || step_q4 > 64) return bad_arg(c);
    return launched(c, svt_hip_launch_convolve8(c->stream, vert, d_src, src_stride, d_dst, dst_stride, d_filters, q0, step_q4, w, h), "convolve8 launch");
}
int svt_hip_wiener_convolve_add_src_dev(SvtHipCtx* c, int pix_bytes, int bd, const void* d_src, int src_stride, void* d_dst, int dst_stride, const int16_t* d_taps, int w, int h,
                                        int round_0, int round_1) {
    SVT_HIP_ENTER(c);
    if (!c || !d_src || !d_dst || !d_taps || w < 1 || h < 1 || !fmt_8to12_ok(pix_bytes, bd) || round_0 < 1 || round_0 > 7 ||
        round_1 < 1 || round_1 > 14)
        return bad_arg(c);
    return launched(c, svt_hip_launch_wiener_convolve(c->stream, pix_bytes, bd, d_src, src_stride, d_dst, dst_stride, d_taps, w, h, round_0, round_1), "wiener convolve launch");
}
int svt_hip_cdef_find_dir_batch_dev(SvtHipCtx* c, const uint16_t* d_img, int stride, const int32_t* d_offs, int n, int coeff_shift, int32_t* d_dir, int32_t* d_var) {
    SVT_HIP_ENTER(c);
    if (!c || !d_img || !d_offs || !d_dir || !d_var || n < 0 || coeff_shift < 0 || coeff_shift > 4) return bad_arg(c);
    return launched(c, svt_hip_launch_cdef_find_dir_list(c->stream, d_img, d_offs, n, stride, coeff_shift, d_dir, d_var), "cdef find dir launch");
}
int svt_hip_cdef_filter_block_batch_dev(SvtHipCtx* c, const uint16_t* d_in, int in_stride, const SvtHipCdefBlk* d_blks, int n, uint8_t* d_dst8, uint16_t* d_dst16,
                                        int dst_stride) {
    SVT_HIP_ENTER(c);
    if (!c || !d_in || !d_blks || n < 0 || (!d_dst8) == (!d_dst16)) return bad_arg(c);
    return launched(c, svt_hip_launch_cdef_filter_block_list(c->stream, d_in, in_stride, d_blks, n, d_dst8, d_dst16, dst_stride), "cdef filter block launch");
}
int svt_hip_lpf_edges_batch_dev(SvtHipCtx* c, int pix_bytes, int bd, void* d_plane, int stride, const SvtHipLpfEdge* d_edges, int n) {
    SVT_HIP_ENTER(c);
    if (!c || !d_plane || !d_edges || n < 0 || !fmt_ok(pix_bytes, bd)) return bad_arg(c);
    return launched(c, svt_hip_launch_lpf_edge_list(c->stream, d_plane, pix_bytes, stride, bd, d_edges, n), "lpf edges launch");
}

}  // extern "C"
