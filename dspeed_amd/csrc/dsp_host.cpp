// dsp_host.cpp -- host half of libdspeed_hip.so: the C ABI of include/dspeed_hip.h.
//
//   * device/memory/stream helpers (thin wrappers so that a host needs nothing but this library);
//   * chain translation: validates a dsp_op program, evaluates every constant the reference evaluates once per
//     call in float64 on the host (exp(-1/tau) through libm exactly as numba/LLVM does, IIR coefficients, lag
//     splits), lays the waveform slots out in LDS and picks the launch geometry.
//
// The single-processor entry points (dsp_<name>_f32 / _f64: tiny cached chains) are clients of this file, in dsp_gufuncs.cpp.
//
// Reference behaviour mirrored here: constant-only DSPFatal conditions are raised at chain creation with the
// reference's own codes/messages (processors/*.py, cited in include/dspeed_hip.h).
#include <hip/hip_runtime.h>

#include <execinfo.h>
#include <signal.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "dsp_gufuncs.h"
#include "dsp_launch.h"
#include "dsp_plan.h"
#include "dsp_spectrum_tables.h"

#define fail dsp_fail
#define elem_size dsp_elem_size

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            (void)hipGetLastError(); /* reported here: do not leave it for an unrelated later launch check */ \
            return fail(DSP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));               \
        }                                                                                          \
    } while (0)

// Release-type calls (free, destroy, unregister) run from destructors / garbage collection at arbitrary moments of the caller: they
// report through their return code only and leave dsp_last_error() alone, so the text of an error the caller is about to read is
// never replaced by an unrelated one.
#define HIP_RELEASE(expr)                       \
    do {                                        \
        hipError_t e_ = (expr);                 \
        if (e_ != hipSuccess) {                 \
            (void)hipGetLastError();            \
            return DSP_ERR_HIP;                 \
        }                                       \
    } while (0)

struct dsp_chain : ChainPlan {
    DevProgram* dev = nullptr;
    size_t dev_bytes = 0;      // bytes of the device copy (the used prefix of DevProgram)
    int* dev_err = nullptr;
    int device = 0;
    int num_cu = 256;
    int64_t f16_rows_cap = 0;
    // dsp_chain_share_row_scales: the pole-zero rows kernel in front writes the scales and flags of the rows it stores straight into this
    // chain's arrays and leaves a note of which rows they describe; dsp_chain_execute checks the note against its own input
    dsp_chain* scale_feeder = nullptr;  // (on the float16 FIR chain)
    dsp_chain* scale_sink = nullptr;    // (on the pole-zero rows chain)
    // the same for a float16 FIR that reads a slice of the rows the pole-zero kernel READS, minus the same baseline column: the kernel sees
    // x - baseline of every sample anyway
    dsp_chain* scale_sink_in = nullptr;  // (on the pole-zero rows chain)
    bool fed_in_side = false;            // (on the FIR chain: the note below describes its rows as the producer's input, fed_bl its baseline)
    const void* fed_bl = nullptr;
    const void* fed_rows_ptr = nullptr;
    void* fed_stream = nullptr;  // the stream of the producer's launch: its scales and flags are ordered ahead of a consumer on that stream only
    int64_t fed_n_wf = -1, fed_stride = 0;
    int32_t fed_len = 0;
    float* cur_scratch = nullptr;  // (current-branch kernel) allocated at the first launch
    int cur_blocks_cap = 0;
    FirRunsTable* runs_table = nullptr;  // (run-length FIR) the kernel's breakpoints, rewritten by every launch; allocated at the first
    float* runs_scratch = nullptr;       // a row per resident wavefront for a filtered waveform that nothing keeps
    void* spec_tables = nullptr;         // (psd, fft) twiddles, unpacking twiddles or chirp, filter: written once by dsp_chain_create, only read after
    // the error word handed to the host by a copy that is part of the launch (dsp_chain_set_async_check): dsp_chain_check then needs no
    // transfer of its own -- one issued while a large host-to-device copy of the next buffer is in flight queues up behind it
    int* err_mirror = nullptr;  // page-locked
    ~dsp_chain() {  // (also on the error paths of dsp_chain_create, which holds the chain in a unique_ptr)
        if (scale_sink) scale_sink->scale_feeder = nullptr;
        if (scale_sink_in) scale_sink_in->scale_feeder = nullptr;
        if (scale_feeder) {
            if (scale_feeder->scale_sink == this) scale_feeder->scale_sink = nullptr;
            if (scale_feeder->scale_sink_in == this) scale_feeder->scale_sink_in = nullptr;
        }
        if (dev) (void)hipFree(dev);
        if (dev_err) (void)hipFree(dev_err);
        if (host.prof) (void)hipFree(host.prof);
        if (err_mirror) (void)hipHostFree(err_mirror);
        if (cur_scratch) (void)hipFree(cur_scratch);
        if (runs_table) (void)hipFree(runs_table);
        if (runs_scratch) (void)hipFree(runs_scratch);
        if (spec_tables) (void)hipFree(spec_tables);
        for (int k = 0; k < DSP_FIR_MAXK; ++k)
            if (f16.taps16[k]) (void)hipFree(const_cast<void*>(f16.taps16[k]));
        if (f16.row_scale) (void)hipFree(const_cast<void*>(f16.row_scale));
        if (f16.row_flags) (void)hipFree(const_cast<void*>(f16.row_flags));
    }
};

// Internal copies between this library's own host structures (programs, error words, tap read-backs) and the device go through one
// page-locked staging buffer: the runtime is never handed heap or stack memory to page-lock on the fly (host memory note).
static std::mutex g_stage_mu;
static void* g_stage = nullptr;
static const size_t STAGE_BYTES = 1 << 20;
static hipError_t stage_ready() {
    if (g_stage) return hipSuccess;
    return hipHostMalloc(&g_stage, STAGE_BYTES, hipHostMallocDefault);
}
static hipError_t staged_h2d(void* dev, const void* host, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_stage_mu);
    hipError_t e = stage_ready();
    for (size_t o = 0; e == hipSuccess && o < bytes; o += STAGE_BYTES) {
        const size_t n = bytes - o < STAGE_BYTES ? bytes - o : STAGE_BYTES;
        memcpy(g_stage, (const char*)host + o, n);
        e = hipMemcpy((char*)dev + o, g_stage, n, hipMemcpyHostToDevice);
    }
    return e;
}
static hipError_t staged_d2h(void* host, const void* dev, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_stage_mu);
    hipError_t e = stage_ready();
    for (size_t o = 0; e == hipSuccess && o < bytes; o += STAGE_BYTES) {
        const size_t n = bytes - o < STAGE_BYTES ? bytes - o : STAGE_BYTES;
        e = hipMemcpy(g_stage, (const char*)dev + o, n, hipMemcpyDeviceToHost);
        if (e == hipSuccess) memcpy((char*)host + o, g_stage, n);
    }
    return e;
}

// the HIP side of the single-processor entry points (dsp_gufuncs.h)
int dsp_gufunc_current_device() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    return dev;
}
int dsp_gufunc_read_back(void* host, const void* dev, size_t bytes) {
    const hipError_t e = staged_d2h(host, dev, bytes);
    if (e == hipSuccess) return DSP_OK;
    (void)hipGetLastError();  // (the text is what the copy reported when it stood in g_convolve)
    return fail(DSP_ERR_HIP, "staged_d2h(taps.data(), kernel_dev, taps.size()) failed: %s", hipGetErrorString(e));
}

// a kernel the chain is planned for that needs more dynamic LDS than a launch gets unasked is told so once, at chain creation
// (`label`: what the error text names, with the bytes where it has a %d)
template <typename Setter>
static int raise_lds(bool planned, int bytes, int limit, const char* label, Setter set) {
    if (!planned || bytes <= limit) return DSP_OK;
    const hipError_t e = (hipError_t)set(bytes);
    if (e == hipSuccess) return DSP_OK;
    char what[64];
    snprintf(what, sizeof what, label, bytes);
    return fail(DSP_ERR_HIP, "hipFuncSetAttribute(%s): %s", what, hipGetErrorString(e));
}

extern "C" {

// ------------------------------------------------------------------------------------------------ device / memory
int dsp_device_count(int* count) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(DSP_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return DSP_OK;
}
int dsp_set_device(int device) {
    HIP_TRY(hipSetDevice(device));
    return DSP_OK;
}
int dsp_get_device(int* device) {
    HIP_TRY(hipGetDevice(device));
    return DSP_OK;
}
int dsp_device_info(int device, char* name, int name_cap, int* compute_units, int64_t* hbm_bytes, int* lds_bytes_per_cu) {
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, device));
    if (name && name_cap > 0) snprintf(name, (size_t)name_cap, "%s (%s)", p.name, p.gcnArchName);
    if (compute_units) *compute_units = p.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)p.totalGlobalMem;
    if (lds_bytes_per_cu) *lds_bytes_per_cu = (int)p.maxSharedMemoryPerMultiProcessor;
    return DSP_OK;
}
int dsp_malloc(void** dev, int64_t bytes) {
    *dev = nullptr;
    HIP_TRY(hipMalloc(dev, (size_t)(bytes > 0 ? bytes : 1)));
    return DSP_OK;
}
int dsp_free(void* dev) {
    if (dev) HIP_RELEASE(hipFree(dev));
    return DSP_OK;
}
int dsp_host_alloc(void** host, int64_t bytes) {
    *host = nullptr;
    HIP_TRY(hipHostMalloc(host, (size_t)(bytes > 0 ? bytes : 1), hipHostMallocDefault));
    return DSP_OK;
}
int dsp_host_free(void* host) {
    if (host) HIP_RELEASE(hipHostFree(host));
    return DSP_OK;
}
int dsp_memset(void* dev, int value, int64_t bytes, void* stream) {
    HIP_TRY(hipMemsetAsync(dev, value, (size_t)bytes, (hipStream_t)stream));
    return DSP_OK;
}
int dsp_h2d(void* dev, const void* host, int64_t bytes) {
    HIP_TRY(hipMemcpy(dev, host, (size_t)bytes, hipMemcpyHostToDevice));
    return DSP_OK;
}
int dsp_d2h(void* host, const void* dev, int64_t bytes) {
    HIP_TRY(hipMemcpy(host, dev, (size_t)bytes, hipMemcpyDeviceToHost));
    return DSP_OK;
}
int dsp_h2d_async(void* dev, const void* host, int64_t bytes, void* stream) {
    HIP_TRY(hipMemcpyAsync(dev, host, (size_t)bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return DSP_OK;
}
int dsp_d2h_async(void* host, const void* dev, int64_t bytes, void* stream) {
    HIP_TRY(hipMemcpyAsync(host, dev, (size_t)bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return DSP_OK;
}
int dsp_stream_create(void** stream) {
    hipStream_t s;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void*)s;
    return DSP_OK;
}
int dsp_stream_destroy(void* stream) {
    HIP_RELEASE(hipStreamDestroy((hipStream_t)stream));
    return DSP_OK;
}
int dsp_stream_sync(void* stream) {
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return DSP_OK;
}
int dsp_sync(void) {
    HIP_TRY(hipDeviceSynchronize());
    return DSP_OK;
}
int dsp_event_create(void** event) {
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    *event = (void*)e;
    return DSP_OK;
}
int dsp_event_destroy(void* event) {
    HIP_RELEASE(hipEventDestroy((hipEvent_t)event));
    return DSP_OK;
}
int dsp_event_record(void* event, void* stream) {
    HIP_TRY(hipEventRecord((hipEvent_t)event, (hipStream_t)stream));
    return DSP_OK;
}
int dsp_stream_wait_event(void* stream, void* event) {
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0));
    return DSP_OK;
}
int dsp_host_register(void* host, int64_t bytes) {
    if (!host || bytes <= 0) return fail(DSP_ERR_ARG, "dsp_host_register: null pointer or empty range");
    hipError_t e = hipHostRegister(host, (size_t)bytes, hipHostRegisterDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // a refusal (range already registered, read-only mapping) must not poison the next launch check
        return fail(DSP_ERR_HIP, "hipHostRegister: %s", hipGetErrorString(e));
    }
    return DSP_OK;
}
int dsp_host_unregister(void* host) {
    if (!host) return DSP_OK;
    hipError_t e = hipHostUnregister(host);
    if (e != hipSuccess) {  // the caller must then keep the memory alive: the runtime still holds a record of the range
        (void)hipGetLastError();
        return fail(DSP_ERR_HIP, "hipHostUnregister: %s", hipGetErrorString(e));
    }
    return DSP_OK;
}
int dsp_event_sync(void* event) {
    HIP_TRY(hipEventSynchronize((hipEvent_t)event));
    return DSP_OK;
}
int dsp_event_elapsed_ms(void* start, void* stop, float* ms) {
    HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return DSP_OK;
}
// Diagnostics: the HIP / ROCr runtimes end the process with abort() on some failures (a GPU memory fault, an internal guarantee)
// without saying where.  With this handler installed SIGABRT first writes the native call stack to stderr, then takes its default
// course.  async-signal-safe calls only (backtrace_symbols_fd writes straight to the descriptor).
static struct sigaction g_prev_abort;
static bool g_abort_installed = false;
static int g_abort_fd = 2;
static void abort_trace_handler(int sig) {
    static const char head[] = "\n[dspeed_hip] SIGABRT -- native call stack of the aborting thread:\n";
    void* frames[64];
    const int n = backtrace(frames, 64);
    (void)!write(g_abort_fd, head, sizeof head - 1);
    backtrace_symbols_fd(frames, n, g_abort_fd);
    if (g_abort_fd != 2) {  // (a test runner may have redirected descriptor 2: say it there as well)
        (void)!write(2, head, sizeof head - 1);
        backtrace_symbols_fd(frames, n, 2);
    }
    // whoever was there before (Python's faulthandler prints its own stack), then the default; never this handler again -- a
    // re-raise into ourselves would loop for ever (the signal is blocked while we run and pends)
    struct sigaction next = g_prev_abort;
    if (!g_abort_installed || next.sa_handler == abort_trace_handler) {
        memset(&next, 0, sizeof next);
        next.sa_handler = SIG_DFL;
        sigemptyset(&next.sa_mask);
    }
    g_abort_installed = false;
    sigaction(sig, &next, nullptr);
    raise(sig);
}
int dsp_install_abort_trace(int fd) {
    g_abort_fd = fd >= 0 ? fd : 2;
    void* warm[2];
    (void)backtrace(warm, 2);  // (loads libgcc's unwinder now, not inside the handler)
    struct sigaction cur;
    if (sigaction(SIGABRT, nullptr, &cur) == 0 && cur.sa_handler == abort_trace_handler) return DSP_OK;  // already there: only the descriptor changed
    struct sigaction sa;
    memset(&sa, 0, sizeof sa);
    sa.sa_handler = abort_trace_handler;
    sigemptyset(&sa.sa_mask);
    struct sigaction prev;
    if (sigaction(SIGABRT, &sa, &prev) != 0) return fail(DSP_ERR_ARG, "sigaction(SIGABRT) failed");
    g_prev_abort = prev;  // the disposition of the FIRST installation is what an uninstall (or the handler) goes back to
    g_abort_installed = true;
    return DSP_OK;
}
int dsp_uninstall_abort_trace(void) {
    struct sigaction cur;
    if (!g_abort_installed || sigaction(SIGABRT, nullptr, &cur) != 0 || cur.sa_handler != abort_trace_handler) {
        g_abort_installed = false;  // (somebody else's handler is in place now: leave it)
        g_abort_fd = 2;
        return DSP_OK;
    }
    g_abort_installed = false;
    g_abort_fd = 2;
    return sigaction(SIGABRT, &g_prev_abort, nullptr) == 0 ? DSP_OK : fail(DSP_ERR_ARG, "sigaction(SIGABRT) failed");
}
const char* dsp_last_error(void) { return dsp_plan_last_error(); }
const char* dsp_version(void) { return "dspeed_hip 0.1 (gfx950)"; }


// The tables of the spectrum kernel (dsp_spectrum_tables.h), float64 on the host, rounded once to the loop's type, in one device block: the
// transform's twiddles, then the unpacking twiddles (a power-of-two row) or the chirp and the filter (Bluestein).  No launch writes them.
static int spectrum_tables(dsp_chain* ch) {
    namespace tb = dsp_spectrum_tables;
    SpectrumArgs& A = ch->only.spec;
    std::vector<double> all = tb::twiddle(A.points);
    const size_t at_aux = all.size();
    const std::vector<double> aux = A.bluestein ? tb::chirp(A.len) : tb::unpack(A.len);
    all.insert(all.end(), aux.begin(), aux.end());
    const size_t at_filter = all.size();
    if (A.bluestein) {
        const std::vector<double> f = tb::filter(A.len, A.points, A.log2_points);
        all.insert(all.end(), f.begin(), f.end());
    }
    const size_t esz = ch->f64 ? 8 : 4;
    std::vector<float> narrow;
    if (!ch->f64) narrow.assign(all.begin(), all.end());
    HIP_TRY(hipMalloc(&ch->spec_tables, all.size() * esz));
    HIP_TRY(staged_h2d(ch->spec_tables, ch->f64 ? (const void*)all.data() : (const void*)narrow.data(), all.size() * esz));
    const char* base = (const char*)ch->spec_tables;
    A.twiddle = base;
    A.aux = base + at_aux * esz;
    A.filter = A.bluestein ? base + at_filter * esz : nullptr;
    return DSP_OK;
}

// ---- the kernel-only routes (dsp_plan.cpp's kernel_only_routes holds what is HIP-free about each): a row per route, at the route's index
struct KernelOnlyLaunch {
    int (*launch)(const KernelOnlyArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream);
    const char* what;
    int (*set_lds)(const dsp_chain* ch, int bytes) = nullptr;  // raises the kernel's dynamic-LDS limit, where the route has one to raise ...
    const char* lds_label = nullptr;                           // ... and what the error text calls it
    // what is the route's own, at most one of the two: device data of the chain, or a pointer no binding stands behind
    int (*at_create)(dsp_chain* ch) = nullptr;
    void (*at_launch)(const dsp_chain* ch, KernelOnlyArgs& A) = nullptr;
};
extern "C++" {
template <typename Args, Args KernelOnlyArgs::*block, int (*launcher)(const Args*, int64_t, int, int, int*, hipStream_t)>
static int launch_block(const KernelOnlyArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream) {
    return launcher(&(A->*block), n_wf, dtype, vec, err, stream);
}
template <int (*setter)(int dtype, int bytes)>
static int set_lds_of_rows(const dsp_chain* ch, int bytes) {
    return setter(ch->only_src.dtype, bytes);
}
}
#define KERNEL_ONLY(Args, block, name) launch_block<Args, &KernelOnlyArgs::block, dsp_internal_launch_##name>
static const KernelOnlyLaunch kernel_only_launches[] = {
    {KERNEL_ONLY(ExtremaArgs, ext, extrema), "extrema kernel launch"},
    {KERNEL_ONLY(HistArgs, hist, hist), "histogram kernel launch"},
    {KERNEL_ONLY(ThreshArgs, thresh, thresh), "threshold kernel launch"},
    {KERNEL_ONLY(SpectrumArgs, spec, spectrum), "spectrum kernel launch", set_lds_of_rows<dsp_internal_set_spectrum_lds>, "spectrum kernel, %d",
     spectrum_tables},  // (the block's table pointers are the chain's)
    {KERNEL_ONLY(SortArgs, sort, sort), "sort kernel launch", set_lds_of_rows<dsp_internal_set_sort_lds>, "sort kernel, %d"},
    {KERNEL_ONLY(InterpArgs, interp, interp), "interp kernel launch", set_lds_of_rows<dsp_internal_set_interp_lds>, "interp kernel, %d"},
    {KERNEL_ONLY(DenseArgs, dense, dense), "dense kernel launch", set_lds_of_rows<dsp_internal_set_dense_lds>, "dense kernel, %d"},
    {KERNEL_ONLY(ReflectArgs, reflect, reflect), "reflect kernel launch", set_lds_of_rows<dsp_internal_set_reflect_lds>, "reflect kernel, %d"},
    {KERNEL_ONLY(PileupArgs, pileup, pileup), "pile-up kernel launch"},
    {KERNEL_ONLY(PulsesArgs, pulses, pulses), "pulse kernel launch"},
    {KERNEL_ONLY(TailfitArgs, tailfit, tailfit), "tail-fit kernel launch"},
    {KERNEL_ONLY(AlignArgs, align, align), "align kernel launch", nullptr, nullptr, nullptr,  // (no LDS)
     [](const dsp_chain* ch, KernelOnlyArgs& A) { A.align.table_nan = A.align.table ? ch->dev_err + DSP_ERR_TABLE_WORD : nullptr; }},
    // (the largest any chain needs, whatever this one does: never lowered under another chain's launch)
    {KERNEL_ONLY(SvmArgs, svm, svm), "svm kernel launch",
     [](const dsp_chain* ch, int) { return dsp_internal_set_svm_lds(ch->only_src.dtype, ch->only.svm.f64, dsp_svm::LDS_MAX); }, "svm kernel, %d"},
};
#undef KERNEL_ONLY
static_assert(sizeof kernel_only_launches / sizeof kernel_only_launches[0] == DSP_KERNEL_ONLY_ROUTES, "a row per kernel-only route, as in dsp_plan.cpp");

int dsp_chain_create(const dsp_op* ops, int n_ops, const dsp_io_desc* io, int n_io, const int32_t* slot_len, int n_slots,
                     int n_sregs, int compute_dtype, dsp_chain** out) {
    if (out) *out = nullptr;
    if (!out) return fail(DSP_ERR_ARG, "null out");
    std::unique_ptr<dsp_chain> ch(new dsp_chain());
    {  // everything that needs no device: validation, constants, LDS packing, kernel choice (dsp_plan.cpp)
        const int rc = dsp_plan_build(ch.get(), ops, n_ops, io, n_io, slot_len, n_slots, n_sregs, compute_dtype);
        if (rc != DSP_OK) return rc;
    }
    const DevProgram& P = ch->host;
    const int esz = (ch->f64 || ch->i64) ? 8 : 4;
    if (ch->fir_f16)  // device images of the float16 FIR's taps (rewritten by every launch: the taps are a binding)
        for (int k = 0; k < ch->fir.n_kernels; ++k) {
            void* buf = nullptr;
            HIP_TRY(hipMalloc(&buf, dsp_fir_f16::taps_bytes(ch->fir.kend)));
            ch->f16.taps16[k] = buf;
        }
    const KernelOnlyLaunch* only = ch->kernel_only != DSP_ROUTE_VM ? &kernel_only_launches[ch->kernel_only] : nullptr;
    if (only && only->at_create)
        if (const int rc = only->at_create(ch.get())) return rc;
    HIP_TRY(hipGetDevice(&ch->device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ch->device));
    ch->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // (the op array is the tail of the structure: only the ops the program has are allocated and uploaded -- 1.5 kB instead of 100 kB
    // for a one-processor chain)
    ch->dev_bytes = offsetof(DevProgram, ops) + (size_t)P.n_ops * sizeof(DevOp);
    HIP_TRY(hipMalloc((void**)&ch->dev, ch->dev_bytes));
    HIP_TRY(staged_h2d(ch->dev, &P, ch->dev_bytes));
    HIP_TRY(hipMalloc((void**)&ch->dev_err, DSP_ERR_WORDS * sizeof(int)));
    HIP_TRY(hipMemset(ch->dev_err, 0, DSP_ERR_WORDS * sizeof(int)));
    const int block_lds = ch->lds_bytes_per_wave * ch->waves_per_block, classic_lds = ch->lds_bytes_per_wave * ch->classic_wpb;
    int rc = raise_lds(ch->kernel_only == DSP_ROUTE_VM, block_lds, 64 * 1024, "MaxDynamicSharedMemorySize=%d", dsp_internal_set_vm_lds);
    if (!rc) rc = raise_lds(ch->fused_ok, classic_lds, 64 * 1024, "energy kernel, %d", [&](int n) { return dsp_internal_set_energy_lds(ch->fused_trap, ch->fused_npf, n); });
    if (!rc) rc = raise_lds(ch->fir_f16, dsp_fir_f16::lds_bytes(), 64 * 1024, "float16 FIR kernel", dsp_internal_set_fir_f16_lds);
    if (!rc) rc = raise_lds(ch->fir_ok, ch->fir_lds_bytes, 64 * 1024, "FIR kernel, %d", ch->fir.store ? dsp_internal_set_fir_store_lds : dsp_internal_set_fir_mfma_lds);
    if (!rc) rc = raise_lds(ch->scalar_ok, n_sregs * 64 * esz, 48 * 1024, "scalar kernel", dsp_internal_set_scalar_lds);
    if (!rc) rc = raise_lds(ch->cur_ok, ch->cur_lds_bytes, 64 * 1024, "current kernel, %d", dsp_internal_set_current_lds);
    if (!rc) rc = raise_lds(ch->rows_ok, ch->rows_lds_bytes, 64 * 1024, "rows kernel, %d", dsp_internal_set_rows_lds);
    if (!rc && only && only->set_lds)
        rc = raise_lds(true, dsp_plan_kernel_only_lds(ch.get()), 64 * 1024, only->lds_label, [&](int n) { return only->set_lds(ch.get(), n); });
    if (rc) return rc;
    *out = ch.release();
    return DSP_OK;
}

// a binding's first element: io_ptrs[k] + offset (the waveform input's offset travels in the kernels' arguments instead)
static void* io_at(const dsp_chain* ch, void* const* io_ptrs, int k) {
    return k < 0 ? nullptr : (void*)((char*)io_ptrs[k] + (int64_t)ch->host.io[k].offset * elem_size(ch->host.io[k].dtype));
}
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Does the kernel of a route run THIS launch?  The program has its shape, the specialised kernels are on, and the buffers of this call keep
// the 16-byte alignment its wide loads need (the plan vouches for strides and offsets, nobody for the pointers).  dsp_chain_execute asks
// in the order of dsp_plan_route; a launch whose planned route does not apply runs on the next that does.
static bool scalar_applies(const dsp_chain* ch, void* const*) { return ch->scalar_ok && ch->fused_on; }
static bool pz_rows_applies(const dsp_chain* ch, void* const* io_ptrs) {
    return ch->pz_ok && ch->fused_on && aligned16(io_ptrs[ch->pio_wf]) && aligned16(io_at(ch, io_ptrs, ch->pio_out));
}
static bool reduce_applies(const dsp_chain* ch, void* const*) { return ch->red_ok && ch->fused_on; }  // (unaligned rows: its scalar loads)
static bool fir_runs_applies(const dsp_chain* ch, void* const* io_ptrs) { return ch->runs_ok && ch->fused_on && aligned16(io_ptrs[ch->uio_wf]); }
static bool current_applies(const dsp_chain* ch, void* const* io_ptrs) { return ch->cur_ok && ch->fused_on && aligned16(io_ptrs[ch->cio_wf]); }
static bool fir_applies(const dsp_chain* ch, void* const* io_ptrs) { return ch->fir_ok && ch->fused_on && aligned16(io_ptrs[ch->fio_wf]); }
// (the rows kernel: the rows and the coefficient buffer of its Haar transform)
static bool rows_applies(const dsp_chain* ch, void* const* io_ptrs) {
    if (!ch->rows_ok || !ch->fused_on || !aligned16(io_ptrs[ch->rio_wf])) return false;
    return ch->rio_dwt < 0 || aligned16((const char*)io_ptrs[ch->rio_dwt] + 4u * (uintptr_t)ch->host.io[ch->rio_dwt].offset);
}
static bool energy_rr_applies(const dsp_chain* ch, void* const* io_ptrs) {
    return ch->rr_ok && ch->fused_on && ch->variant != 1 && aligned16(io_ptrs[ch->io_wf]);
}
static bool energy_applies(const dsp_chain* ch, void* const* io_ptrs) { return ch->fused_ok && ch->fused_on && aligned16(io_ptrs[ch->io_wf]); }

static int chain_blocks(const dsp_chain* ch, int64_t n_wf, int wpb, int cap_waves) {
    const int block_lds = ch->lds_bytes_per_wave * wpb;
    int per_cu = LDS_BYTES_PER_CU / block_lds;
    if (per_cu > cap_waves / wpb) per_cu = cap_waves / wpb;
    if (per_cu < 1) per_cu = 1;
    int64_t want = (n_wf + wpb - 1) / wpb;
    int64_t cap = (int64_t)ch->num_cu * per_cu;
    int64_t b = want < cap ? want : cap;
    return (int)(b > 0 ? b : 1);
}
static int vm_blocks(const dsp_chain* ch, int64_t n_wf) { return chain_blocks(ch, n_wf, ch->waves_per_block, ch->has_fir ? 8 : 12); }

// launch geometry of the register-resident kernel: up to 4 wavefronts per block, 2 wavefronts per SIMD (its register budget)
static void rr_geometry(const dsp_chain* ch, int64_t n_wf, int* wpb_out, int* blocks_out) {
    int wpb = LDS_BYTES_PER_CU / ch->rr_lds_bytes;
    if (wpb > 4) wpb = 4;
    if (wpb < 1) wpb = 1;
    if (const char* env = getenv("DSPEED_HIP_WPB")) {  // tuning knob: wavefronts per workgroup
        const int v = atoi(env);
        if (v >= 1 && v <= wpb) wpb = v;
    }
    int per_cu = LDS_BYTES_PER_CU / (ch->rr_lds_bytes * wpb);
    if (per_cu * wpb > 8) per_cu = 8 / wpb;
    if (per_cu < 1) per_cu = 1;
    const int64_t want = (n_wf + wpb - 1) / wpb, cap = (int64_t)ch->num_cu * per_cu;
    *wpb_out = wpb;
    *blocks_out = (int)(want < cap ? want : cap);
}

// launch geometry of the current-branch kernel (dsp_current.hip): persistent wavefronts, as many as a CU's LDS takes (at most 12 per CU) ...
static int current_blocks_cap(const dsp_chain* ch) {
    int per_cu = LDS_BYTES_PER_CU / ch->cur_lds_bytes;
    if (per_cu > 12) per_cu = 12;  // (three wavefronts per SIMD: the kernel's 109 - 163 registers allow them)
    return ch->num_cu * (per_cu < 1 ? 1 : per_cu);
}
// ... and of those as many as make every one walk the same number of 64-row groups (2 048 groups on 1 280 wavefronts are two rounds, the
// second three fifths empty; on 1 024 they are two full ones with a wavefront less per CU in each other's way).  One helper for the launch
// and for dsp_chain_geometry.
static int current_blocks(const dsp_chain* ch, int64_t n_wf) {
    const int64_t groups = (n_wf + 63) / 64, cap = current_blocks_cap(ch);
    const int64_t rounds = (groups + cap - 1) / cap;
    return (int)((groups + rounds - 1) / (rounds < 1 ? 1 : rounds));
}

// launch geometry of the run-length FIR (dsp_fir_runs.hip): persistent workgroups of four wavefronts, a row per wavefront and round; four
// workgroups per CU where LDS allows (the kernel's registers leave room for five wavefronts per SIMD), every one the same number of rounds
static int runs_blocks_cap(const dsp_chain* ch) {
    int per_cu = LDS_BYTES_PER_CU / dsp_fir_runs::lds_bytes(ch->runs.m);
    if (per_cu > 4) per_cu = 4;
    return ch->num_cu * (per_cu < 1 ? 1 : per_cu);
}
static int runs_blocks(const dsp_chain* ch, int64_t n_wf) {
    const int64_t groups = (n_wf + 3) / 4, cap = runs_blocks_cap(ch);
    const int64_t rounds = (groups + cap - 1) / cap;
    return (int)((groups + rounds - 1) / (rounds < 1 ? 1 : rounds));
}

// makes `device` current for the calling thread and puts the previous one back when it goes out of scope
struct DeviceScope {
    int prev = -1;
    bool switched = false, ok = true;
    explicit DeviceScope(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) {
            ok = hipSetDevice(device) == hipSuccess;
            switched = ok;
        }
    }
    ~DeviceScope() {
        if (switched && prev >= 0) (void)hipSetDevice(prev);
    }
};

static int post_err(dsp_chain* ch, void* stream) {
    if (ch->err_mirror) HIP_TRY(hipMemcpyAsync(ch->err_mirror, ch->dev_err, 4 * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    return DSP_OK;
}

// the rows' scales and flags of a float16 FIR chain: grown to the largest batch seen
static int f16_rows_reserve(dsp_chain* ch, int64_t n_wf) {
    if (ch->f16_rows_cap >= n_wf) return DSP_OK;
    if (ch->f16.row_scale) HIP_TRY(hipFree(const_cast<void*>(ch->f16.row_scale)));
    if (ch->f16.row_flags) HIP_TRY(hipFree(const_cast<void*>(ch->f16.row_flags)));
    ch->f16.row_scale = ch->f16.row_flags = nullptr;
    ch->f16_rows_cap = 0;
    void *a = nullptr, *b = nullptr;
    HIP_TRY(hipMalloc(&a, (size_t)n_wf * sizeof(float)));
    ch->f16.row_scale = a;
    HIP_TRY(hipMalloc(&b, (size_t)n_wf * sizeof(unsigned)));
    ch->f16.row_flags = b;
    ch->f16_rows_cap = n_wf;
    return DSP_OK;
}

int dsp_chain_share_row_scales(dsp_chain* producer, dsp_chain* consumer) {
    if (!producer || !consumer || producer == consumer) return fail(DSP_ERR_ARG, "dsp_chain_share_row_scales: two chains");
    if (!producer->pz_ok || !consumer->fir_ok || !consumer->fir_f16 || producer->device != consumer->device || consumer->scale_feeder) return 0;
    if (consumer->fir.in_kind == 0 && consumer->fir.sub_mode == 0 && !producer->scale_sink) {  // the FIR reads the rows the kernel writes
        producer->scale_sink = consumer;
        consumer->scale_feeder = producer;
        consumer->fed_in_side = false;
        return 1;
    }
    // the FIR reads a slice of the rows the kernel reads, minus the same baseline column: integer rows only (a float32 row's NaN rule looks at the
    // samples around the slice as well); that the two are bound to the same buffers is checked at every execute
    const PzArgs& P = producer->pz;
    const FirArgs& F = consumer->fir;
    if (F.in_kind != 0 && F.in_kind == P.in_kind && F.sub_mode == 1 && P.sub_mode == 1 && consumer->fio_bl >= 0 && producer->pio_bl >= 0 &&
        F.wf_stride == P.wf_stride && F.bl_stride == P.bl_stride && F.wf_offset >= P.wf_offset && F.wf_offset + F.n <= P.wf_offset + P.len &&
        !producer->scale_sink_in) {
        producer->scale_sink_in = consumer;
        consumer->scale_feeder = producer;
        consumer->fed_in_side = true;
        return 1;
    }
    return 0;
}

// the outputs, pick-offs and walks of ReduceArgs: the reduce kernel's own and the ones the run-length FIR runs on its filtered rows
static void bind_reductions(const dsp_chain* ch, void* const* io_ptrs, ReduceArgs& A) {
    auto at = [&](int k) { return io_at(ch, io_ptrs, k); };
    for (int k = 0; k < 5; ++k) A.out[k] = at(ch->dio_out[k]);
    for (int k = 0; k < DSP_REDUCE_PICKS; ++k) A.pick_out[k] = at(ch->dio_pick[k]);
    for (int k = 0; k < DSP_REDUCE_WALKS; ++k) {
        A.walk_out[k] = at(ch->dio_walk[k]);
        A.walk_thr[k] = (const float*)at(ch->dio_walk_thr[k]);
        A.walk_ts[k] = (const float*)at(ch->dio_walk_ts[k]);
    }
}

// ---- one launch per route: the kernel's argument block with the pointers of this call, its launch, the error word on its way to the host
static int launched(dsp_chain* ch, void* stream, hipError_t e, const char* what) {
    if (e != hipSuccess) return fail(DSP_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    return post_err(ch, stream);
}

// the shared ending of the kernels that stream rows (dsp_row_stream.h): 16-byte loads where the plan vouches for strides, offsets and length
// and this call's pointer for the alignment
extern "C++" template <typename Args, typename Launcher>
static int launch_on_rows(dsp_chain* ch, int64_t n_wf, void* stream, const Args& A, const RowSource& src, Launcher launcher, const char* what) {
    const int vec = src.vec && aligned16(A.wf);
    hipError_t e = (hipError_t)launcher(&A, n_wf, src.dtype, vec, ch->dev_err, (hipStream_t)stream);
    return launched(ch, stream, e, what);
}

// the one launch of them all: the plan's block with this call's pointers (dsp_internal_plan_fill_args, which the CPU tests check), the
// route's own, the kernel
static int launch_kernel_only(dsp_chain* ch, void* const* io_ptrs, int64_t n_wf, void* stream) {
    const KernelOnlyLaunch& r = kernel_only_launches[ch->kernel_only];
    KernelOnlyArgs A;
    dsp_internal_plan_fill_args(ch, io_ptrs, &A);
    if (r.at_launch) r.at_launch(ch, A);
    return launch_on_rows(ch, n_wf, stream, A, ch->only_src, r.launch, r.what);
}

static int launch_scalar(dsp_chain* ch, const IoPtrs* ptrs, int64_t n_wf, void* stream) {
    hipError_t e = (hipError_t)dsp_internal_launch_scalar(ch->dev, ptrs, n_wf, ch->host.n_sregs, ch->i64 ? 2 : (ch->f64 ? 1 : 0), (hipStream_t)stream);
    return launched(ch, stream, e, "scalar kernel launch");
}

static int launch_pz_rows(dsp_chain* ch, void* const* io_ptrs, int64_t n_wf, void* stream) {
    auto at = [&](int k) { return io_at(ch, io_ptrs, k); };
    PzArgs A = ch->pz;
    A.wf = io_ptrs[ch->pio_wf];
    A.bl = (const float*)at(ch->pio_bl);
    A.out = at(ch->pio_out);
    A.tau = (const float*)at(ch->pio_tau);
    for (int k = 0; k < 4; ++k) A.mm_out[k] = at(ch->pio_mm[k]);
    A.row_scale = nullptr;
    A.row_flags = nullptr;
    if (dsp_chain* sink = ch->scale_sink) {
        const int rc = f16_rows_reserve(sink, n_wf);
        if (rc != DSP_OK) return rc;
        A.row_scale = (float*)const_cast<void*>(sink->f16.row_scale);
        A.row_flags = (uint32_t*)const_cast<void*>(sink->f16.row_flags);
        sink->fed_rows_ptr = A.out;
        sink->fed_stream = stream;
        sink->fed_n_wf = n_wf;
        sink->fed_stride = A.out_stride;
        sink->fed_len = A.len;
    }
    A.in_scale = nullptr;
    A.in_flags = nullptr;
    if (dsp_chain* sink = ch->scale_sink_in) {
        const int rc = f16_rows_reserve(sink, n_wf);
        if (rc != DSP_OK) return rc;
        const int es = A.in_kind == 0 ? 4 : 2;
        A.in_scale = (float*)const_cast<void*>(sink->f16.row_scale);
        A.in_flags = (uint32_t*)const_cast<void*>(sink->f16.row_flags);
        A.in_lo = sink->fir.wf_offset - A.wf_offset;
        A.in_hi = A.in_lo + sink->fir.n;
        sink->fed_rows_ptr = (const char*)A.wf + (size_t)sink->fir.wf_offset * es;  // the consumer's first sample, if it is bound to these rows
        sink->fed_bl = A.bl;
        sink->fed_stream = stream;
        sink->fed_n_wf = n_wf;
        sink->fed_stride = A.wf_stride;
        sink->fed_len = sink->fir.n;
    }
    hipError_t e = (hipError_t)dsp_internal_launch_pz_rows(&A, n_wf, ch->dev_err, (hipStream_t)stream);
    return launched(ch, stream, e, "pole-zero rows kernel launch");
}

static int launch_reduce(dsp_chain* ch, void* const* io_ptrs, int64_t n_wf, void* stream) {
    ReduceArgs A = ch->red;
    A.wf = io_ptrs[ch->red_src.io];
    bind_reductions(ch, io_ptrs, A);
    return launch_on_rows(ch, n_wf, stream, A, ch->red_src, dsp_internal_launch_reduce, "reduce kernel launch");
}

static int launch_fir_runs(dsp_chain* ch, void* const* io_ptrs, int64_t n_wf, void* stream) {
    auto at = [&](int k) { return io_at(ch, io_ptrs, k); };
    if (!ch->runs_table) HIP_TRY(hipMalloc((void**)&ch->runs_table, sizeof(FirRunsTable)));
    FirRunsArgs A = ch->runs;
    if (!A.keep && !ch->runs_scratch)
        HIP_TRY(hipMalloc((void**)&ch->runs_scratch, (size_t)runs_blocks_cap(ch) * 4 * (size_t)A.out_stride * sizeof(float)));
    A.wf = (const float*)io_ptrs[ch->uio_wf];
    A.taps = (const float*)at(ch->uio_taps);
    A.out = A.keep ? (float*)at(ch->uio_out) : ch->runs_scratch;
    A.table = ch->runs_table;
    bind_reductions(ch, io_ptrs, A.red);
    hipError_t e = (hipError_t)dsp_internal_launch_fir_runs(&A, ch->runs_table, n_wf, runs_blocks(ch, n_wf), ch->dev_err, (hipStream_t)stream);
    return launched(ch, stream, e, "run-length FIR kernel launch");
}

static int launch_current(dsp_chain* ch, void* const* io_ptrs, int64_t n_wf, void* stream) {
    auto at = [&](int k) { return io_at(ch, io_ptrs, k); };
    // persistent wavefronts, as many as a CU's LDS takes (at most 12 per CU): each keeps its scratch area for the groups of rows it walks
    const int cap = current_blocks_cap(ch);
    if (!ch->cur_scratch) {
        HIP_TRY(hipMalloc((void**)&ch->cur_scratch, (size_t)cap * (size_t)ch->cur.scratch_per_wave * sizeof(float)));
        ch->cur_blocks_cap = cap;
    }
    CurrentArgs A = ch->cur;
    A.wf = io_ptrs[ch->cio_wf];
    A.t0 = (const float*)at(ch->cio_t0);
    for (int k = 0; k < 4; ++k) A.out[k] = at(ch->cio_out[k]);
    A.scratch = ch->cur_scratch;
    const int blocks = current_blocks(ch, n_wf);
    hipError_t e = (hipError_t)dsp_internal_launch_current(&A, n_wf, blocks, ch->cur_lds_bytes, (hipStream_t)stream);
    return launched(ch, stream, e, "current kernel launch");
}

static int launch_fir(dsp_chain* ch, void* const* io_ptrs, int64_t n_wf, void* stream) {
    auto at = [&](int k) { return io_at(ch, io_ptrs, k); };
    FirArgs A = ch->fir;
    A.wf = io_ptrs[ch->fio_wf];
    A.bl = (const float*)at(ch->fio_bl);
    for (int k = 0; k < A.n_kernels; ++k) {
        A.taps[k] = (const float*)at(ch->fio_taps[k]);
        A.out[k] = at(ch->fio_out[k]);
    }
    if (ch->fir_f16) {
        const int rc = f16_rows_reserve(ch, n_wf);
        if (rc != DSP_OK) return rc;
        // scales and flags already there?  Only if the kernel in front wrote exactly the rows this one reads, and just now
        const void* first = (const char*)A.wf + (size_t)A.wf_offset * (A.in_kind == 0 ? sizeof(float) : sizeof(int16_t));
        // -- and on this stream: scales and flags are written by the producer's launch, so only stream order puts them ahead of this one
        const bool same_batch = ch->scale_feeder && ch->fed_rows_ptr == first && ch->fed_n_wf == n_wf && ch->fed_stream == stream &&
                                ch->fed_stride == A.wf_stride && ch->fed_len == A.n;
        ch->f16.rows_done = (same_batch && (ch->fed_in_side ? (A.in_kind != 0 && A.sub_mode == 1 && ch->fed_bl == (const void*)A.bl && A.bl != nullptr)
                                                            : (A.in_kind == 0 && A.sub_mode == 0))) ? 1 : 0;
        ch->fed_n_wf = -1;  // (a note is good for one execute)
    }
    hipError_t e = (hipError_t)(ch->fir_f16 ? dsp_internal_launch_fir_f16(&A, &ch->f16, n_wf, dsp_fir_f16::lds_bytes(), (hipStream_t)stream)
                                : A.store   ? dsp_internal_launch_fir_store(&A, n_wf, ch->fir_lds_bytes, (hipStream_t)stream)
                                            : dsp_internal_launch_fir_mfma(&A, n_wf, ch->fir_lds_bytes, (hipStream_t)stream));
    return launched(ch, stream, e, "FIR kernel launch");
}

static int launch_rows(dsp_chain* ch, void* const* io_ptrs, int64_t n_wf, void* stream) {
    auto at = [&](int k) { return io_at(ch, io_ptrs, k); };
    RowsArgs A = ch->rows;
    A.wf = io_ptrs[ch->rio_wf];
    A.bl = (const float*)at(ch->rio_bl);
    A.thr = (const float*)at(ch->rio_thr);
    A.ts = (const float*)at(ch->rio_ts);
    for (int k = 0; k < 4; ++k) A.out_mm[k] = at(ch->rio_mm[k]);
    A.out_tpt = at(ch->rio_tpt);
    A.dwt_out = at(ch->rio_dwt);
    hipError_t e = (hipError_t)dsp_internal_launch_rows(&A, n_wf, ch->dev_err, ch->rows_lds_bytes, (hipStream_t)stream);
    return launched(ch, stream, e, "rows kernel launch");
}

static int launch_energy_rr(dsp_chain* ch, void* const* io_ptrs, int64_t n_wf, void* stream) {
    auto at = [&](int k) { return io_at(ch, io_ptrs, k); };
    EnergyArgs F = ch->rr;
    F.wf = io_ptrs[ch->io_wf];
    F.bl = (const float*)at(ch->io_bl);
    F.tp = (const float*)at(ch->io_tp);
    F.tau = (const float*)at(ch->io_tau);
    F.out = (float*)at(ch->io_out);
    const int S = (ch->variant == 8 && ch->wf_dtype == DSP_F32) ? 2 : 1;
    int rwpb, rblocks;
    rr_geometry(ch, n_wf, &rwpb, &rblocks);
    hipError_t e = (hipError_t)dsp_internal_launch_energy_rr(&F, &ch->plan[S - 1], ch->fused_trap, ch->fused_npf, S, ch->wf_dtype, n_wf,
                                                             ch->dev_err, rblocks, 64 * rwpb, ch->rr_lds_bytes * rwpb, (hipStream_t)stream);
    return launched(ch, stream, e, "energy kernel launch");
}

static int launch_energy(dsp_chain* ch, void* const* io_ptrs, int64_t n_wf, void* stream) {
    auto at = [&](int k) { return io_at(ch, io_ptrs, k); };
    EnergyArgs F = ch->fused;
    F.wf = io_ptrs[ch->io_wf];
    F.bl = (const float*)at(ch->io_bl);
    F.tp = (const float*)at(ch->io_tp);
    F.out = (float*)at(ch->io_out);
    const int cw = ch->classic_wpb;
    hipError_t e = (hipError_t)dsp_internal_launch_energy(&F, ch->fused_trap, ch->fused_npf, n_wf, ch->dev_err, chain_blocks(ch, n_wf, cw, 8),
                                                          64 * cw, ch->lds_bytes_per_wave * cw, (hipStream_t)stream);
    return launched(ch, stream, e, "energy kernel launch");
}

static int launch_vm(dsp_chain* ch, const IoPtrs* ptrs, int64_t n_wf, void* stream) {
    const int blocks = vm_blocks(ch, n_wf);
    const int threads = 64 * ch->waves_per_block;
    const int lds = ch->lds_bytes_per_wave * ch->waves_per_block;
    hipError_t e = ch->f64 ? (hipError_t)dsp_internal_launch_vm_f64(ch->dev, ptrs, n_wf, ch->dev_err, blocks, threads, lds, ch->has_fir,
                                                                    (hipStream_t)stream)
                           : (hipError_t)dsp_internal_launch_vm_f32(ch->dev, ptrs, n_wf, ch->dev_err, blocks, threads * ch->host.team, lds, ch->has_fir,
                                                                    ch->host.team, (hipStream_t)stream);
    return launched(ch, stream, e, "kernel launch");
}

int dsp_chain_execute(dsp_chain* ch, void* const* io_ptrs, int64_t n_wf, void* stream) {
    if (!ch || !io_ptrs) return fail(DSP_ERR_ARG, "null chain or io_ptrs");
    if (n_wf <= 0) return DSP_OK;
    IoPtrs ptrs{};
    for (int k = 0; k < ch->host.n_io; ++k) {
        if (!io_ptrs[k]) return fail(DSP_ERR_ARG, "io binding %d is NULL", k);
        ptrs.p[k] = io_ptrs[k];
    }
    DeviceScope on_chain_device(ch->device);  // the chain's program and error word live there; the caller's current device comes back on return
    if (!on_chain_device.ok) return fail(DSP_ERR_HIP, "hipSetDevice(%d) failed", ch->device);
    (void)hipGetLastError();  // launch checks below report this launch, not a stale error of an unrelated earlier call
    // the first kernel, in the order of dsp_plan_route, that takes this launch's pointers
    if (ch->kernel_only != DSP_ROUTE_VM) return launch_kernel_only(ch, io_ptrs, n_wf, stream);  // (always: the program runs nowhere else; unaligned rows: the kernel's scalar loads)
    if (scalar_applies(ch, io_ptrs)) return launch_scalar(ch, &ptrs, n_wf, stream);
    if (pz_rows_applies(ch, io_ptrs)) return launch_pz_rows(ch, io_ptrs, n_wf, stream);
    if (reduce_applies(ch, io_ptrs)) return launch_reduce(ch, io_ptrs, n_wf, stream);
    if (fir_runs_applies(ch, io_ptrs)) return launch_fir_runs(ch, io_ptrs, n_wf, stream);
    if (current_applies(ch, io_ptrs)) return launch_current(ch, io_ptrs, n_wf, stream);
    if (fir_applies(ch, io_ptrs)) return launch_fir(ch, io_ptrs, n_wf, stream);  // (float16, kept output or float32 amax form)
    if (rows_applies(ch, io_ptrs)) return launch_rows(ch, io_ptrs, n_wf, stream);
    if (energy_rr_applies(ch, io_ptrs)) return launch_energy_rr(ch, io_ptrs, n_wf, stream);
    if (energy_applies(ch, io_ptrs)) return launch_energy(ch, io_ptrs, n_wf, stream);
    return launch_vm(ch, &ptrs, n_wf, stream);
}

int dsp_chain_check(dsp_chain* ch, void* stream, int64_t* row) {
    if (!ch) return fail(DSP_ERR_ARG, "null chain");
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    int host_err[DSP_ERR_WORDS] = {0};
    if (ch->err_mirror) {
        memcpy(host_err, ch->err_mirror, 4 * sizeof(int));  // (copied by the launch itself, on its stream)
    } else {
        HIP_TRY(staged_d2h(host_err, ch->dev_err, sizeof host_err));
    }
#ifdef DSPEED_HIP_DIAG
    if (getenv("DSPEED_HIP_ABLATE") && (atoi(getenv("DSPEED_HIP_ABLATE")) & 8)) {  // diagnostic phase stamps
        unsigned long long ph[6];
        memcpy(ph, host_err + 4, sizeof ph);
        unsigned long long tot = 0;
        for (int i = 0; i < 6; ++i) tot += ph[i];
        if (tot) {
            fprintf(stderr, "[dspeed_hip stamps] cycles per phase (stage, pass1, pass2, carries, pass3, tail):");
            for (int i = 0; i < 6; ++i) fprintf(stderr, " %.1f%%", 100.0 * (double)ph[i] / (double)tot);
            fprintf(stderr, "  total %llu\n", tot);
            HIP_TRY(hipMemset(ch->dev_err + 4, 0, sizeof ph));
        }
    }
#endif
    if (host_err[0] != 0) {
        if (row) *row = ((int64_t)(uint32_t)host_err[2] << 32) | (uint32_t)host_err[1];
        if (ch->err_mirror) memset(ch->err_mirror, 0, 4 * sizeof(int));  // consumed: a second check without a launch in between reports nothing
        HIP_TRY(hipMemsetAsync(ch->dev_err, 0, 4 * sizeof(int), (hipStream_t)stream));  // (in stream order, ahead of the next launch)
        dsp_set_last_error(dsp_fatal_message(host_err[0]));
        return host_err[0];
    }
    return DSP_OK;
}

int dsp_chain_profile(dsp_chain* ch, int enable) {
    if (!ch) return fail(DSP_ERR_ARG, "null chain");
    HIP_TRY(hipSetDevice(ch->device));
    const size_t bytes = (size_t)(ch->host.n_ops + 1) * sizeof(unsigned long long);
    if (enable) {
        if (!ch->host.prof) HIP_TRY(hipMalloc((void**)&ch->host.prof, bytes));
        HIP_TRY(hipMemset(ch->host.prof, 0, bytes));
    } else if (ch->host.prof) {
        HIP_RELEASE(hipFree(ch->host.prof));
        ch->host.prof = nullptr;
    }
    HIP_TRY(staged_h2d(ch->dev, &ch->host, ch->dev_bytes));
    return DSP_OK;
}

int dsp_chain_profile_read(dsp_chain* ch, int capacity, int32_t* opcodes, int32_t* slots, uint64_t* cycles, int* n_ops, uint64_t* n_waveforms) {
    if (!ch || !n_ops) return fail(DSP_ERR_ARG, "null argument");
    *n_ops = ch->host.n_ops;
    if (!ch->host.prof) return fail(DSP_ERR_ARG, "profiling is off: call dsp_chain_profile(chain, 1) and execute first");
    if (capacity < ch->host.n_ops || !opcodes || !cycles || !slots) return fail(DSP_ERR_ARG, "capacity %d < %d ops", capacity, ch->host.n_ops);
    HIP_TRY(hipSetDevice(ch->device));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<unsigned long long> host(ch->host.n_ops + 1);
    HIP_TRY(staged_d2h(host.data(), ch->host.prof, host.size() * sizeof(unsigned long long)));
    for (int i = 0; i < ch->host.n_ops; ++i) {
        opcodes[i] = ch->host.ops[i].opcode;
        slots[i] = ch->host.ops[i].src;
        cycles[i] = host[i];
    }
    if (n_waveforms) *n_waveforms = host[ch->host.n_ops];
    return DSP_OK;
}

int dsp_chain_destroy(dsp_chain* ch) {
    if (!ch) return DSP_OK;
    delete ch;
    return DSP_OK;
}

int dsp_chain_geometry(dsp_chain* ch, int64_t n_wf, int* lds_bytes_per_wave, int* waves_per_block, int* blocks) {
    if (!ch) return fail(DSP_ERR_ARG, "null chain");
    int lds = 0, wpb = 0, b = 0;
    switch (dsp_plan_route(ch)) {
        case DSP_ROUTE_SCALAR:
            lds = ch->host.n_sregs * 64 * ((ch->f64 || ch->i64) ? 8 : 4), wpb = 1, b = (int)((n_wf + 63) / 64);
            break;
        case DSP_ROUTE_PZ_ROWS:
        case DSP_ROUTE_REDUCE: lds = 0, wpb = 4, b = (int)((n_wf + 3) / 4); break;
        case DSP_ROUTE_FIR_RUNS: lds = dsp_fir_runs::lds_bytes(ch->runs.m) / 4, wpb = 4, b = runs_blocks(ch, n_wf); break;
        case DSP_ROUTE_CURRENT: lds = ch->cur_lds_bytes, wpb = 1, b = current_blocks(ch, n_wf); break;
        case DSP_ROUTE_FIR_F16:
        case DSP_ROUTE_FIR_STORE:
        case DSP_ROUTE_FIR_MFMA:  // 8 wavefronts per 64 waveforms and kernel
            lds = ch->fir_lds_bytes / 8, wpb = 8, b = (int)((n_wf + 63) / 64) * (ch->fir.store ? (ch->fir.p[0] + 319) / 320 : ch->fir.n_kernels);
            break;
        case DSP_ROUTE_ROWS:  // a pair of wavefronts per 64 waveforms shares one history ring
            lds = ch->rows_lds_bytes / 2, wpb = 2, b = (int)((n_wf + 63) / 64);
            break;
        case DSP_ROUTE_ENERGY_RR:
            rr_geometry(ch, n_wf, &wpb, &b);
            lds = ch->rr_lds_bytes;
            break;
        case DSP_ROUTE_ENERGY:  // (reported as the interpreter's: the classic kernel runs on its LDS layout)
        case DSP_ROUTE_VM:
            lds = ch->lds_bytes_per_wave / ch->host.team;  // (a team of wavefronts shares a row's image)
            wpb = ch->waves_per_block * ch->host.team, b = vm_blocks(ch, n_wf);
            break;
        // the kernel-only routes, one case: a row each of the planner's table (no default: a new route without a case is a compiler warning)
        case DSP_ROUTE_EXTREMA: case DSP_ROUTE_HIST: case DSP_ROUTE_THRESH: case DSP_ROUTE_SPECTRUM: case DSP_ROUTE_SORT: case DSP_ROUTE_INTERP: case DSP_ROUTE_DENSE:
        case DSP_ROUTE_REFLECT: case DSP_ROUTE_PILEUP: case DSP_ROUTE_PULSES: case DSP_ROUTE_TAILFIT: case DSP_ROUTE_ALIGN: case DSP_ROUTE_SVM:
            dsp_plan_kernel_only_geometry(ch, n_wf, &lds, &wpb, &b);
            break;
    }
    if (lds_bytes_per_wave) *lds_bytes_per_wave = lds;
    if (waves_per_block) *waves_per_block = wpb;
    if (blocks) *blocks = b;
    return DSP_OK;
}

const char* dsp_chain_kernel_name(dsp_chain* ch) { return dsp_plan_kernel_name(ch); }

const char* dsp_chain_kernel_note(dsp_chain* ch) {
    if (!ch) return "";
    return dsp_plan_specialised(ch) ? "" : ch->note.c_str();
}

int dsp_chain_set_async_check(dsp_chain* ch, int enable) {
    if (!ch) return fail(DSP_ERR_ARG, "null chain");
    if (enable && !ch->err_mirror) {
        HIP_TRY(hipHostMalloc((void**)&ch->err_mirror, DSP_ERR_WORDS * sizeof(int), hipHostMallocDefault));
        memset(ch->err_mirror, 0, DSP_ERR_WORDS * sizeof(int));
    } else if (!enable && ch->err_mirror) {
        (void)hipHostFree(ch->err_mirror);
        ch->err_mirror = nullptr;
    }
    return DSP_OK;
}

int dsp_chain_set_fused(dsp_chain* ch, int enable) {
    if (!ch) return fail(DSP_ERR_ARG, "null chain");
    ch->fused_on = (enable & 1) != 0;  // bit 0: use a specialised kernel
    // bits 1-3 pick one for cross-checks and A/B runs: 0 = default (register-resident where it applies), 6 = register-resident,
    // 7 = classic (VM layout); anything else = default
    const int v = (enable >> 1) & 7;
    ch->variant = (v == 7 || !ch->rr_ok) ? 1 : 6;
    return dsp_plan_specialised(ch) ? 1 : 0;
}

int dsp_stream_read(const void* src, int64_t bytes, void* sink, void* stream) {
    if (!src || !sink || bytes < 16) return fail(DSP_ERR_ARG, "dsp_stream_read: need a source of at least 16 bytes and a 4-byte sink");
    if (reinterpret_cast<uintptr_t>(src) & 15u) return fail(DSP_ERR_ARG, "dsp_stream_read: source must be 16-byte aligned");
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    const int cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    hipError_t e = (hipError_t)dsp_internal_launch_stream_read(src, bytes, (uint32_t*)sink, cus * 8, (hipStream_t)stream);
    if (e != hipSuccess) return fail(DSP_ERR_HIP, "stream-read kernel launch failed: %s", hipGetErrorString(e));
    return DSP_OK;
}

int dsp_synth_waveforms(void* wf, int out_dtype, int64_t n_wf, int32_t wf_len, int64_t row_stride, float* baseline, float* t_pick,
                        uint64_t seed, int64_t first_row, float tau, float sigma, float pick_offset, float bl_lo, float bl_hi,
                        float amp_lo, float amp_hi, void* stream) {
    if (out_dtype != DSP_F32 && out_dtype != DSP_I16) return fail(DSP_ERR_ARG, "synth output must be float32 or int16");
    if (n_wf <= 0) return DSP_OK;
    hipError_t e = (hipError_t)dsp_internal_launch_synth(wf, out_dtype, n_wf, wf_len, row_stride, baseline, t_pick, seed, first_row, tau,
                                                         sigma, pick_offset, bl_lo, bl_hi, amp_lo, amp_hi, 1.0f, 1.0f, (hipStream_t)stream);
    if (e != hipSuccess) return fail(DSP_ERR_HIP, "synth launch failed: %s", hipGetErrorString(e));
    return DSP_OK;
}

int dsp_synth_pulses(void* wf, int out_dtype, int64_t n_wf, int32_t wf_len, int64_t row_stride, float* baseline, float* t_pick, uint64_t seed,
                     int64_t first_row, float tau, float sigma, float pick_offset, float bl_lo, float bl_hi, float amp_lo, float amp_hi,
                     float rise_lo, float rise_hi, void* stream) {
    if (out_dtype != DSP_F32 && out_dtype != DSP_I16) return fail(DSP_ERR_ARG, "synth output must be float32 or int16");
    if (!(rise_lo >= 1.0f) || !(rise_hi >= rise_lo)) return fail(DSP_ERR_ARG, "synth: rise times are 1 <= rise_lo <= rise_hi samples");
    if (n_wf <= 0) return DSP_OK;
    hipError_t e = (hipError_t)dsp_internal_launch_synth(wf, out_dtype, n_wf, wf_len, row_stride, baseline, t_pick, seed, first_row, tau,
                                                         sigma, pick_offset, bl_lo, bl_hi, amp_lo, amp_hi, rise_lo, rise_hi, (hipStream_t)stream);
    if (e != hipSuccess) return fail(DSP_ERR_HIP, "synth launch failed: %s", hipGetErrorString(e));
    return DSP_OK;
}

int dsp_linear_slope_fit_rows(const void* wf, int wf_dtype, int64_t n_wf, int32_t wf_len, int64_t row_stride, int compute_dtype,
                              const void* sub_dev, int sub_dtype, double sub_const, int sub_mode, int has_pz, double pz_tau,
                              const dsp_fit_window* fits, int n_fits, void* out, void* stream) {
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64) return fail(DSP_ERR_ARG, "compute_dtype must be DSP_F32 or DSP_F64");
    const bool f64 = compute_dtype == DSP_F64;
    if (!elem_size(wf_dtype) || wf_dtype == DSP_BOOL) return fail(DSP_ERR_ARG, "fit rows: unknown waveform dtype %d", wf_dtype);
    if (!f64 && (wf_dtype == DSP_I32 || wf_dtype == DSP_U32 || wf_dtype == DSP_F64))
        return fail(DSP_ERR_ARG, "fit rows: int32/uint32/float64 rows select the float64 loop (compute_dtype DSP_F64)");
    if (!fits || n_fits < 1 || n_fits > DSP_FIT_MAX) return fail(DSP_ERR_ARG, "fit rows: n_fits=%d out of range (1..%d)", n_fits, DSP_FIT_MAX);
    if (sub_mode < 0 || sub_mode > 2) return fail(DSP_ERR_ARG, "fit rows: sub_mode must be 0, 1 (bl_subtract) or 2 (numpy.subtract)");
    if (sub_mode && sub_dev && (!elem_size(sub_dtype) || sub_dtype == DSP_BOOL)) return fail(DSP_ERR_ARG, "fit rows: unknown dtype of the subtracted column");
    if (n_wf < 0 || wf_len <= 0 || row_stride < wf_len || (n_wf > 0 && (!wf || !out))) return fail(DSP_ERR_ARG, "fit rows: bad rows / buffers");
    FitArgs A;
    memset(&A, 0, sizeof A);
    A.wf = wf;
    A.n_wf = n_wf;
    A.row_stride = row_stride;
    A.wf_len = wf_len;
    A.sub = sub_mode ? sub_dev : nullptr;
    A.sub_dtype = sub_dtype;
    A.sub_mode = sub_mode;
    A.sub_const = f64 ? sub_const : (double)(float)sub_const;
    A.has_pz = has_pz ? 1 : 0;
    if (has_pz) {  // the constant as the chain's POLE_ZERO op forms it: the loop's scalar type, then exp(-1 / tau) in float64 through libm
        const double tau = f64 ? pz_tau : (double)(float)pz_tau;
        A.pz_nan = std::isnan(tau) ? 1 : 0;
        A.pz_c = std::exp(-1.0 / tau);
    }
    A.n_fits = n_fits;
    int max_end = 0;
    bool whole = sub_mode == 1;
    for (int k = 0; k < n_fits; ++k) {
        const dsp_fit_window& w = fits[k];
        if (w.stage < 0 || w.stage > 1 || (w.stage == 1 && !has_pz)) return fail(DSP_ERR_ARG, "fit rows: window %d: stage 1 is the pole-zero corrected waveform (has_pz)", k);
        if (w.first < 0 || w.count < 1 || (int64_t)w.first + w.count > wf_len) return fail(DSP_ERR_ARG, "fit rows: window %d is not inside the waveform", k);
        // one sample: the line fit's denominator is 0 (linear_slope_fit.py raises ZeroDivisionError) -- refused as the in-chain op refuses it
        if (w.count < 2) return fail(DSP_E_ZERODIV, "%s", dsp_fatal_message(DSP_E_ZERODIV));
        A.stage[k] = w.stage;
        A.first[k] = w.first;
        A.count[k] = w.count;
        if (w.first + w.count > max_end) max_end = w.first + w.count;
        whole |= w.stage == 1;
    }
    A.n_scan = whole ? wf_len : max_end;  // (the NaN rules of bl_subtract and pole_zero look at the whole waveform)
    A.out = out;
    if (n_wf == 0) return DSP_OK;
    hipError_t e = (hipError_t)dsp_internal_launch_fit_rows(&A, wf_dtype, compute_dtype, (hipStream_t)stream);
    if (e != hipSuccess) return fail(DSP_ERR_HIP, "fit rows launch failed: %s", hipGetErrorString(e));
    return DSP_OK;
}

}  // extern "C"
