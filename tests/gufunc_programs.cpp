// gufunc_programs.cpp -- the single-processor entry points (dspeed_amd/csrc/dsp_gufuncs.cpp) on the CPU, under AddressSanitizer and
// UndefinedBehaviorSanitizer: every exported dsp_<name>_f32 / _f64 is called with tiny arguments against stand-ins for the chain functions
// and the two host seams, and the program each call builds, the io pointers it hands over and what it returns are printed, one text record
// per call.  tests/test_gufunc_programs_cpu.py compares the output with tests/golden/gufunc_programs.txt.gz, exactly.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tests/gufunc_programs.cpp
//       dspeed_amd/csrc/dsp_gufuncs.cpp dspeed_amd/csrc/dsp_plan.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <set>
#include <vector>

#include "../dspeed_amd/csrc/dsp_gufuncs.h"
#include "../dspeed_amd/csrc/dsp_plan.h"
#include "dspeed_hip.h"

// ------------------------------------------------------------------------------------------------ stand-ins
struct dsp_chain {
    int id, n_io;
};

namespace {

// the caller's arguments: every pointer an entry point is given points into one of these, so that an io pointer is printed as name+bytes
struct Named {
    const char* name;
    const void* base;
    size_t bytes;
};
std::vector<Named> g_named;
bool g_quiet = false;  // (the cache-overflow loop: counted, not printed)
std::set<dsp_chain*> g_live;  // (the library keeps its cached chains until the process ends: main releases them for LeakSanitizer)
int g_next_id = 0, g_creates = 0, g_executes = 0, g_checks = 0, g_destroys = 0;

void print_ptr(const void* p) {
    if (!p) {
        printf("null");
        return;
    }
    for (const Named& n : g_named) {
        const char* b = (const char*)n.base;
        if ((const char*)p >= b && (const char*)p < b + n.bytes) {
            printf("%s+%td", n.name, (const char*)p - b);
            return;
        }
    }
    printf("?");
}

unsigned long long bits(double v) {
    unsigned long long u;
    memcpy(&u, &v, 8);
    return u;
}

}  // namespace

extern "C" {

int dsp_chain_create(const dsp_op* ops, int n_ops, const dsp_io_desc* io, int n_io, const int32_t* slot_len, int n_slots, int n_sregs,
                     int compute_dtype, dsp_chain** out) {
    *out = new dsp_chain{g_next_id++, n_io};
    g_live.insert(*out);
    ++g_creates;
    if (g_quiet) return DSP_OK;
    printf("  create #%d type=%d n_sregs=%d slots=[", (*out)->id, compute_dtype, n_sregs);
    for (int s = 0; s < n_slots; ++s) printf("%s%d", s ? " " : "", slot_len[s]);
    printf("]\n");
    for (int k = 0; k < n_io; ++k)
        printf("    io %d: kind=%d dtype=%d len=%d offset=%d stride=%lld\n", k, io[k].kind, io[k].dtype, io[k].len, io[k].offset,
               (long long)io[k].row_stride);
    for (int k = 0; k < n_ops; ++k) {
        const dsp_op& o = ops[k];
        printf("    op %d: opcode=%d dst=%d src=%d io=%d ip=[%d %d %d %d] sp=[", k, o.opcode, o.dst, o.src, o.io, o.ip[0], o.ip[1], o.ip[2], o.ip[3]);
        for (int j = 0; j < 4; ++j) printf("%s%d:%d:%016llx", j ? " " : "", o.sp[j].kind, o.sp[j].index, bits(o.sp[j].value));
        printf("]\n");
    }
    return DSP_OK;
}

int dsp_chain_execute(dsp_chain* chain, void* const* io_ptrs, int64_t n_wf, void* stream) {
    ++g_executes;
    if (g_quiet) return DSP_OK;
    printf("  execute #%d n_wf=%lld stream=", chain->id, (long long)n_wf);
    print_ptr(stream);
    printf(" ptrs=[");
    for (int k = 0; k < chain->n_io; ++k) {  // (one per io descriptor; a vector too short is AddressSanitizer's to find)
        if (k) printf(" ");
        print_ptr(io_ptrs[k]);
    }
    printf("]\n");
    return DSP_OK;
}

int dsp_chain_check(dsp_chain* chain, void* stream, int64_t* row) {
    ++g_checks;
    if (g_quiet) return DSP_OK;
    printf("  check #%d stream=", chain->id);
    print_ptr(stream);
    printf(" row=");
    print_ptr(row);
    printf("\n");
    return DSP_OK;
}

int dsp_chain_destroy(dsp_chain* chain) {
    ++g_destroys;
    if (!g_quiet) printf("  destroy #%d\n", chain->id);
    g_live.erase(chain);
    delete chain;
    return DSP_OK;
}

}  // extern "C"

int dsp_gufunc_current_device() { return 0; }
int dsp_gufunc_read_back(void* host, const void* dev, size_t bytes) {
    printf("  read_back ");
    print_ptr(dev);
    printf(" bytes=%zu\n", bytes);
    memcpy(host, dev, bytes);
    return DSP_OK;
}

// ------------------------------------------------------------------------------------------------ the calls
namespace {

template <typename FT>
struct Api;
#define API(SFX, FT, TY) \
    template <> \
    struct Api<FT> { \
        static constexpr const char* sfx = #SFX; \
        static constexpr int ty = TY; \
        static constexpr auto bl_subtract = dsp_bl_subtract_##SFX; \
        static constexpr auto pole_zero = dsp_pole_zero_##SFX; \
        static constexpr auto pole_zero_col = dsp_pole_zero_col_##SFX; \
        static constexpr auto double_pole_zero = dsp_double_pole_zero_##SFX; \
        static constexpr auto double_pole_zero_col = dsp_double_pole_zero_col_##SFX; \
        static constexpr auto trap_filter = dsp_trap_filter_##SFX; \
        static constexpr auto trap_norm = dsp_trap_norm_##SFX; \
        static constexpr auto asym_trap_filter = dsp_asym_trap_filter_##SFX; \
        static constexpr auto fixed_time_pickoff = dsp_fixed_time_pickoff_##SFX; \
        static constexpr auto time_point_thresh = dsp_time_point_thresh_##SFX; \
        static constexpr auto interpolated_time_point_thresh = dsp_interpolated_time_point_thresh_##SFX; \
        static constexpr auto min_max_norm = dsp_min_max_norm_##SFX; \
        static constexpr auto windower = dsp_windower_##SFX; \
        static constexpr auto avg_current = dsp_avg_current_##SFX; \
        static constexpr auto trap_pickoff = dsp_trap_pickoff_##SFX; \
        static constexpr auto upsampler = dsp_upsampler_##SFX; \
        static constexpr auto moving_window_multi = dsp_moving_window_multi_##SFX; \
        static constexpr auto linear_slope_fit = dsp_linear_slope_fit_##SFX; \
        static constexpr auto mean_below_threshold = dsp_mean_below_threshold_##SFX; \
        static constexpr auto min_max = dsp_min_max_##SFX; \
        static constexpr auto dwt_haar = dsp_dwt_haar_##SFX; \
        static constexpr auto convolve_wf = dsp_convolve_wf_##SFX; \
        static constexpr auto get_multi_local_extrema = dsp_get_multi_local_extrema_##SFX; \
        static constexpr auto histogram = dsp_histogram_##SFX; \
        static constexpr auto histogram_stats = dsp_histogram_stats_##SFX; \
        static constexpr auto multi_time_point_thresh = dsp_multi_time_point_thresh_##SFX; \
        static constexpr auto time_over_threshold = dsp_time_over_threshold_##SFX; \
    };
API(f32, float, DSP_F32)
API(f64, double, DSP_F64)
#undef API

const char* g_sfx = "";
int64_t g_n = 0;
#define CALL(label, expr) \
    do { \
        if (!g_quiet) printf("%s_%s n_wf=%lld\n", label, g_sfx, (long long)g_n); \
        const int rc_ = (expr); \
        if (!g_quiet) { \
            printf("  -> %d", rc_); \
            if (rc_) printf(" \"%s\"", dsp_plan_last_error()); \
            printf("\n"); \
        } \
    } while (0)

constexpr int N_WF = 3, LEN = 16;

// every entry point of one loop type on `n` rows of LEN samples; (pointer, value) pairs once as a column and once as a constant
template <typename FT>
void calls(int64_t n) {
    using A = Api<FT>;
    g_sfx = A::sfx;
    g_n = n;
    static FT rows[N_WF * LEN], out[N_WF * LEN], out2[N_WF * LEN], c0[N_WF], c1[N_WF], c2[N_WF], c3[N_WF], s0[N_WF], s1[N_WF], s2[N_WF], s3[N_WF];
    static FT taps[4], thr[N_WF * 4];
    static int16_t rows16[N_WF * LEN];
    static uint32_t n0[N_WF], n1[N_WF];
    static char stream_mem[1];
    static int64_t row;
    g_named = {{"rows", rows, sizeof rows}, {"out", out, sizeof out}, {"out2", out2, sizeof out2}, {"c0", c0, sizeof c0}, {"c1", c1, sizeof c1},
               {"c2", c2, sizeof c2}, {"c3", c3, sizeof c3}, {"s0", s0, sizeof s0}, {"s1", s1, sizeof s1}, {"s2", s2, sizeof s2},
               {"s3", s3, sizeof s3}, {"taps", taps, sizeof taps}, {"thr", thr, sizeof thr}, {"rows16", rows16, sizeof rows16},
               {"n0", n0, sizeof n0}, {"n1", n1, sizeof n1}, {"stream", stream_mem, 1}, {"row", &row, sizeof row}};
    void* st = stream_mem;
    int64_t* er = &row;
    const int ty = A::ty;
    const FT none = 0;  // the value beside a column

    CALL("bl_subtract/column", A::bl_subtract(rows, ty, n, LEN, LEN, c0, none, out, LEN, st, er));
    CALL("bl_subtract/column again", A::bl_subtract(rows, ty, n, LEN, LEN, c1, none, out2, LEN, st, er));  // the cached chain, other pointers
    CALL("bl_subtract/constant", A::bl_subtract(rows, ty, n, LEN, LEN, nullptr, (FT)0.1, out, LEN, st, er));
    CALL("bl_subtract/int16 rows", A::bl_subtract(rows16, DSP_I16, n, LEN, LEN, nullptr, (FT)2, out, LEN + 2, nullptr, nullptr));
    CALL("pole_zero", A::pole_zero(rows, ty, n, LEN, LEN, (FT)1716.28, out, LEN, st, er));
    CALL("pole_zero_col/column", A::pole_zero_col(rows, ty, n, LEN, LEN, c0, none, out, LEN, st, er));
    CALL("pole_zero_col/constant", A::pole_zero_col(rows, ty, n, LEN, LEN, nullptr, (FT)100, out, LEN, st, er));
    CALL("double_pole_zero", A::double_pole_zero(rows, ty, n, LEN, LEN, (FT)100, (FT)10, (FT)0.25, out, LEN, st, er));
    CALL("double_pole_zero_col/columns", A::double_pole_zero_col(rows, ty, n, LEN, LEN, c0, none, c1, none, c2, none, out, LEN, st, er));
    CALL("double_pole_zero_col/constants", A::double_pole_zero_col(rows, ty, n, LEN, LEN, nullptr, (FT)100, nullptr, (FT)10, nullptr, (FT)0.25, out, LEN, st, er));
    CALL("double_pole_zero_col/mixed", A::double_pole_zero_col(rows, ty, n, LEN, LEN, nullptr, (FT)100, c1, none, nullptr, (FT)0.25, out, LEN, st, er));
    CALL("trap_filter", A::trap_filter(rows, ty, n, LEN, LEN, 4, 2, out, LEN, st, er));
    CALL("trap_norm", A::trap_norm(rows, ty, n, LEN, LEN, 4, 2, out, LEN, st, er));
    CALL("asym_trap_filter", A::asym_trap_filter(rows, ty, n, LEN, LEN, 4, 2, 3, out, LEN, st, er));
    CALL("fixed_time_pickoff/column", A::fixed_time_pickoff(rows, ty, n, LEN, LEN, c0, none, 'i', s0, st, er));
    CALL("fixed_time_pickoff/constant", A::fixed_time_pickoff(rows, ty, n, LEN, LEN, nullptr, (FT)7.5, 'l', s0, st, er));
    CALL("time_point_thresh/columns", A::time_point_thresh(rows, ty, n, LEN, LEN, c0, none, c1, none, (FT)1, s0, st, er));
    CALL("time_point_thresh/constants", A::time_point_thresh(rows, ty, n, LEN, LEN, nullptr, (FT)0.5, nullptr, (FT)12, (FT)0, s0, st, er));
    CALL("interpolated_time_point_thresh/columns", A::interpolated_time_point_thresh(rows, ty, n, LEN, LEN, c0, none, c1, none, 1, 'l', s0, st, er));
    CALL("interpolated_time_point_thresh/constants", A::interpolated_time_point_thresh(rows, ty, n, LEN, LEN, nullptr, (FT)0.5, nullptr, (FT)12, 0, 'n', s0, st, er));
    CALL("interpolated_time_point_thresh/mode 0", A::interpolated_time_point_thresh(rows, ty, n, LEN, LEN, c0, none, c1, none, 1, 0, s0, st, er));
    CALL("interpolated_time_point_thresh/mode 200", A::interpolated_time_point_thresh(rows, ty, n, LEN, LEN, c0, none, c1, none, 1, 200, s0, st, er));
    CALL("min_max_norm/columns", A::min_max_norm(rows, ty, n, LEN, LEN, c0, none, c1, none, out, LEN, st, er));
    CALL("min_max_norm/constants", A::min_max_norm(rows, ty, n, LEN, LEN, nullptr, (FT)-2, nullptr, (FT)3, out, LEN, st, er));
    CALL("windower/column", A::windower(rows, ty, n, LEN, LEN, c0, none, out, 8, 8, st, er));
    CALL("windower/constant", A::windower(rows, ty, n, LEN, LEN, nullptr, (FT)3, out, 8, 8, st, er));
    CALL("avg_current", A::avg_current(rows, ty, n, LEN, LEN, (FT)10, out, 6, 6, st, er));
    CALL("trap_pickoff/column", A::trap_pickoff(rows, ty, n, LEN, LEN, 4, 2, c0, none, s0, st, er));
    CALL("trap_pickoff/constant", A::trap_pickoff(rows, ty, n, LEN, LEN, 4, 2, nullptr, (FT)11, s0, st, er));
    CALL("upsampler", A::upsampler(rows, ty, n, LEN, LEN, (FT)0.5, out, 8, 8, st, er));
    CALL("moving_window_multi/one", A::moving_window_multi(rows, ty, n, LEN, LEN, (FT)3, (FT)1, 0, out, LEN, st, er));
    CALL("moving_window_multi/two", A::moving_window_multi(rows, ty, n, LEN, LEN, (FT)3, (FT)2, 1, out, LEN, st, er));
    CALL("moving_window_multi/one and a half", A::moving_window_multi(rows, ty, n, LEN, LEN, (FT)3, (FT)1.5, 0, out, LEN, st, er));
    CALL("linear_slope_fit", A::linear_slope_fit(rows, ty, n, LEN, LEN, s0, s1, s2, s3, st, er));
    CALL("mean_below_threshold/column", A::mean_below_threshold(rows, ty, n, LEN, LEN, c0, none, s0, st, er));
    CALL("mean_below_threshold/constant", A::mean_below_threshold(rows, ty, n, LEN, LEN, nullptr, (FT)0.75, s0, st, er));
    CALL("min_max", A::min_max(rows, ty, n, LEN, LEN, s0, s1, s2, s3, st, er));
    CALL("dwt_haar", A::dwt_haar(rows, ty, n, LEN, LEN, 1, 'a', out, 8, 8, st, er));
    taps[0] = 1, taps[1] = (FT)-0.5, taps[2] = (FT)0.25, taps[3] = 2;
    CALL("convolve_wf/clean taps", A::convolve_wf(rows, ty, n, LEN, LEN, taps, 4, 'v', out, 13, 13, st, er));
    CALL("convolve_wf/no output", A::convolve_wf(rows, ty, n, LEN, LEN, taps, 4, 'v', out, 0, 0, st, er));
    taps[2] = std::numeric_limits<FT>::quiet_NaN();
    CALL("convolve_wf/NaN tap", A::convolve_wf(rows, ty, n, LEN, LEN, taps, 4, 'f', out, 8, 8, st, er));
    taps[2] = -std::numeric_limits<FT>::infinity();
    CALL("convolve_wf/Inf tap", A::convolve_wf(rows, ty, n, LEN, LEN, taps, 4, 's', out, 8, 8, st, er));
    taps[1] = std::numeric_limits<FT>::quiet_NaN();
    CALL("convolve_wf/NaN and Inf taps", A::convolve_wf(rows, ty, n, LEN, LEN, taps, 4, 's', out, 8, 8, st, er));
    CALL("convolve_wf/empty kernel", A::convolve_wf(rows, ty, n, LEN, LEN, taps, 0, 'v', out, 8, 8, st, er));
    CALL("get_multi_local_extrema/columns", A::get_multi_local_extrema(rows, ty, n, LEN, LEN, c0, none, c1, none, 3, c2, none, c3, none, out, out2, 5, 5, n0, n1, st, er));
    CALL("get_multi_local_extrema/constants", A::get_multi_local_extrema(rows, ty, n, LEN, LEN, nullptr, (FT)0.5, nullptr, (FT)0.25, 0, nullptr, (FT)1, nullptr, (FT)-1, out, out2, 5, 5, n0, n1, st, er));
    CALL("histogram", A::histogram(rows, ty, n, LEN, LEN, out, 4, 4, out2, 5, 5, st, er));
    CALL("histogram/no bins", A::histogram(rows, ty, n, LEN, LEN, out, 0, 0, out2, 5, 5, st, er));
    CALL("histogram_stats/column", A::histogram_stats(out, n, 4, 4, out2, 5, 5, c0, none, s0, s1, s2, st, er));
    CALL("histogram_stats/constant", A::histogram_stats(out, n, 4, 4, out2, 5, 5, nullptr, (FT)NAN, s0, s1, s2, st, er));
    CALL("histogram_stats/no bins", A::histogram_stats(out, n, 0, 4, out2, 5, 5, nullptr, (FT)NAN, s0, s1, s2, st, er));
    CALL("multi_time_point_thresh/one list", A::multi_time_point_thresh(rows, ty, n, LEN, LEN, thr, 4, 0, c0, none, (FT)1, 'i', out, 4, st, er));
    CALL("multi_time_point_thresh/a list per row", A::multi_time_point_thresh(rows, ty, n, LEN, LEN, thr, 4, 4, nullptr, (FT)6, (FT)-1, 'l', out, 4, st, er));
    CALL("multi_time_point_thresh/no threshold", A::multi_time_point_thresh(rows, ty, n, LEN, LEN, thr, 0, 0, c0, none, (FT)1, 'i', out, 0, st, er));
    CALL("multi_time_point_thresh/null thresholds", A::multi_time_point_thresh(rows, ty, n, LEN, LEN, nullptr, 4, 0, c0, none, (FT)1, 'i', out, 4, st, er));
    CALL("multi_time_point_thresh/negative count", A::multi_time_point_thresh(rows, ty, n, LEN, LEN, thr, -1, 0, c0, none, (FT)1, 'i', out, 4, st, er));
    CALL("time_over_threshold/column", A::time_over_threshold(rows, ty, n, LEN, LEN, c0, none, s0, st, er));
    CALL("time_over_threshold/constant", A::time_over_threshold(rows, ty, n, LEN, LEN, nullptr, (FT)0.5, s0, st, er));
}

// more distinct programs than the cache holds (256): it is emptied, its chains destroyed, and the entry that made it overflow kept
template <typename FT>
void overflow_the_cache() {
    using A = Api<FT>;
    static FT rows[N_WF * 400], out[N_WF * 400];
    g_quiet = true;
    const int before[4] = {g_creates, g_executes, g_checks, g_destroys};
    for (int len = 20; len < 320; ++len) CALL("", A::trap_filter(rows, A::ty, N_WF, len, len, 4, 2, out, len, nullptr, nullptr));
    g_quiet = false;
    printf("cache overflow %s: 300 programs, creates=%d executes=%d checks=%d destroys=%d\n", A::sfx, g_creates - before[0], g_executes - before[1],
           g_checks - before[2], g_destroys - before[3]);
    g_sfx = A::sfx, g_n = N_WF;
    g_named = {{"rows", rows, sizeof rows}, {"out", out, sizeof out}};
    CALL("trap_filter/still cached after the overflow", A::trap_filter(rows, A::ty, N_WF, 319, 319, 4, 2, out, 319, nullptr, nullptr));
    CALL("trap_filter/dropped by the overflow", A::trap_filter(rows, A::ty, N_WF, 20, 20, 4, 2, out, 20, nullptr, nullptr));
}

}  // namespace

int main() {
    calls<float>(N_WF);
    calls<double>(N_WF);
    calls<float>(0);  // the early exits, and which refusals come before them
    calls<double>(0);
    calls<float>(N_WF);  // every program again: one create, two executes
    overflow_the_cache<float>();
    overflow_the_cache<double>();
    printf("totals: creates=%d executes=%d checks=%d destroys=%d live=%zu\n", g_creates, g_executes, g_checks, g_destroys, g_live.size());
    for (dsp_chain* ch : g_live) delete ch;
    return 0;
}
