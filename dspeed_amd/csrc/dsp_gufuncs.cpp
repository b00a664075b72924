// dsp_gufuncs.cpp -- the single-processor entry points of include/dspeed_hip.h (dsp_<name>_f32 / _f64): each is a tiny cached chain.
//
// A pure client of dsp_chain_create / execute / check / destroy.  The two things it needs from the HIP side -- the current device, for the
// cache key, and the read-back of a convolution's taps -- come through dsp_gufuncs.h, so this file includes no HIP header and is also
// compiled for the CPU with -fsanitize=address,undefined against stand-ins (tests/gufunc_programs.cpp, tests/test_gufunc_programs_cpu.py:
// the program every entry point builds is compared with a recording there).
//
// One implementation per processor, generic in the loop type TY (DSP_F32 / DSP_F64); the exported dsp_<name>_f32 / _f64 functions at the
// end only fix the scalar C types.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/dspeed_hip.h"
#include "dsp_gufuncs.h"
#include "dsp_plan.h"

namespace {

struct MiniKey {
    std::vector<int64_t> v;
    bool operator<(const MiniKey& o) const { return v < o.v; }
};
std::map<MiniKey, dsp_chain*> g_cache;
std::mutex g_cache_mu;

int64_t dbits(double f) {
    int64_t i;
    memcpy(&i, &f, 8);
    return i;
}

struct WfIn {  // rows read
    const void* ptr;
    int dtype;
    int64_t n_wf;
    int32_t len;
    int64_t stride;
};
struct WfOut {  // rows written, of the loop type
    void* ptr;
    int32_t len;
    int64_t stride;
};
struct Col {  // scalar gufunc argument: device column (of the loop type) if given, else broadcast constant
    const void* dev;
    double value;
};
using Ints = std::initializer_list<int32_t>;
using Cols = std::initializer_list<Col>;

struct Mini {
    int ty;  // DSP_F32 or DSP_F64: the gufunc loop
    std::vector<dsp_op> ops;
    std::vector<dsp_io_desc> io;
    std::vector<void*> ptrs;
    std::vector<int32_t> slots;
    int n_sregs = 0;
    MiniKey key;

    explicit Mini(int ty_) : ty(ty_) { key.v.push_back(ty_); }

    int add_io(int kind, int dtype, int len, int64_t stride, const void* p) {
        dsp_io_desc d{kind, dtype, len, 0, stride};
        io.push_back(d);
        ptrs.push_back(const_cast<void*>(p));
        key.v.insert(key.v.end(), {kind, dtype, len, stride});
        return (int)io.size() - 1;
    }
    int add_slot(int len) {
        key.v.push_back(len);
        slots.push_back(len);
        return (int)slots.size() - 1;
    }
    dsp_op& add_op(int opcode, int dst, int src, int io_idx) {
        dsp_op o;
        memset(&o, 0, sizeof o);
        o.opcode = opcode;
        o.dst = dst;
        o.src = src;
        o.io = io_idx;
        ops.push_back(o);
        key.v.insert(key.v.end(), {opcode, dst, src, io_idx});
        return ops.back();
    }
    dsp_scalar_arg scalar(const Col& c) {
        dsp_scalar_arg a{DSP_ARG_CONST, 0, c.value};
        if (c.dev) {
            a.kind = DSP_ARG_INPUT;
            a.index = add_io(DSP_IO_SCALAR_IN, ty, 1, 1, c.dev);
        } else {
            key.v.push_back(dbits(c.value));
        }
        return a;
    }
    // the verbs the processors below are written in.  load: rows into `slot`, a new one unless given
    int load(const WfIn& in, int slot = -1) {
        if (slot < 0) slot = add_slot(in.len);
        add_op(DSP_OP_LOAD, slot, 0, add_io(DSP_IO_WF_IN, in.dtype, in.len, in.stride, in.ptr));
        return slot;
    }
    // an op with its integer parameters and scalar operands (their columns are bound before the op is added)
    dsp_op& op(int opcode, int dst, int src, int io_idx, Ints ip = {}, Cols sp = {}) {
        dsp_scalar_arg a[4];
        int n = 0;
        for (const Col& c : sp) a[n++] = scalar(c);
        dsp_op& o = add_op(opcode, dst, src, io_idx);
        std::copy(ip.begin(), ip.end(), o.ip);
        std::copy(a, a + n, o.sp);
        return o;
    }
    void store(int slot, const WfOut& out) { add_op(DSP_OP_STORE, 0, slot, add_io(DSP_IO_WF_OUT, ty, out.len, out.stride, out.ptr)); }
    // scalar register k to a column of `dtype`
    void store_scalar(int k, void* out, int dtype) { add_op(DSP_OP_STORE_SCALAR, 0, 0, add_io(DSP_IO_SCALAR_OUT, dtype, 1, 1, out)).ip[0] = k; }

    int run(int64_t n_wf, void* stream, int64_t* err_row) {
        for (auto& o : ops) {
            for (int k = 0; k < 4; ++k) key.v.push_back(o.ip[k]);
            key.v.push_back(o.io);
        }
        // The cached chains carry one device error word each and are destroyed when the cache is emptied: look-up, creation, execution and
        // the check of the error word happen under the cache's lock, so the dsp_<name>_f32/_f64 entry points are serialised within a
        // process (threads that want concurrency build their own chains with dsp_chain_create).
        std::lock_guard<std::mutex> lk(g_cache_mu);
        key.v.push_back(dsp_gufunc_current_device());
        key.v.push_back((int64_t)dsp_plan_switches());  // (a chain planned under other routing switches is another chain)
        dsp_chain* ch = nullptr;
        auto it = g_cache.find(key);
        if (it != g_cache.end()) ch = it->second;
        if (!ch) {
            int rc = dsp_chain_create(ops.data(), (int)ops.size(), io.data(), (int)io.size(), slots.data(), (int)slots.size(), n_sregs, ty,
                                      &ch);
            if (rc) return rc;
            if (g_cache.size() > 256) {  // (nobody is inside a cached chain: we hold the lock)
                for (auto& kv : g_cache) dsp_chain_destroy(kv.second);
                g_cache.clear();
            }
            g_cache[key] = ch;
        }
        int rc = dsp_chain_execute(ch, ptrs.data(), n_wf, stream);
        if (rc) return rc;
        return dsp_chain_check(ch, stream, err_row);
    }
};

// The frame of every processor: nothing to do without rows; otherwise `build` writes the program (or refuses the arguments) and it runs.
template <typename Build>
int tiny_chain(int ty, int64_t n_wf, void* stream, int64_t* err_row, Build build) {
    if (n_wf <= 0) return DSP_OK;
    Mini m(ty);
    if (int rc = build(m)) return rc;
    return m.run(n_wf, stream, err_row);
}

// waveform -> waveform processors
int wf2wf(int ty, int opcode, const WfIn& in, Ints ip, Cols sp, const WfOut& out, void* st, int64_t* er) {
    return tiny_chain(ty, in.n_wf, st, er, [&](Mini& m) {
        // the per-sample and scan filters work in place: one LDS slot, so a wavefront holds a waveform twice as long (about 38 k float32
        // samples instead of 19 k for the filters that need source and destination side by side)
        const bool in_place = (opcode == DSP_OP_BL_SUBTRACT || opcode == DSP_OP_POLE_ZERO || opcode == DSP_OP_DOUBLE_POLE_ZERO) && out.len == in.len;
        const int s_in = m.add_slot(in.len), s_out = in_place ? s_in : m.add_slot(out.len);
        m.load(in, s_in);
        m.op(opcode, s_out, s_in, 0, ip, sp);
        m.store(s_out, out);
        return DSP_OK;
    });
}

// waveform -> scalars processors: the op leaves a value per output in the scalar registers, register k goes to outs[k]
int wf2scalars(int ty, int opcode, const WfIn& in, Ints ip, Cols sp, std::initializer_list<void*> outs, void* st, int64_t* er) {
    return tiny_chain(ty, in.n_wf, st, er, [&](Mini& m) {
        m.n_sregs = (int)outs.size();
        m.op(opcode, 0, m.load(in), 0, ip, sp);
        int k = 0;
        for (void* out : outs) m.store_scalar(k++, out, ty);
        return DSP_OK;
    });
}

int g_min_max_norm(int ty, const WfIn& in, const Col& lo, const Col& hi, const WfOut& out, void* st, int64_t* er) {
    return tiny_chain(ty, in.n_wf, st, er, [&](Mini& m) {
        const int s = m.load(in);
        m.op(DSP_OP_MIN_MAX_NORM, s, s, 0, {}, {lo, hi});  // in place
        m.store(s, out);
        return DSP_OK;
    });
}

int g_convolve(int ty, const WfIn& in, const void* kernel_dev, int32_t kernel_len, int32_t mode, const WfOut& out, void* st, int64_t* er) {
    return tiny_chain(ty, in.n_wf, st, er, [&](Mini& m) -> int {
        if (kernel_len <= 0) return dsp_fail(DSP_ERR_ARG, "empty kernel");
        // NaN among the taps -> NaN output (convolutions.py:45-46): look at them once on the host
        const size_t esz = ty == DSP_F64 ? 8 : 4;
        std::vector<unsigned char> taps(esz * (size_t)kernel_len);
        if (int rc = dsp_gufunc_read_back(taps.data(), kernel_dev, taps.size())) return rc;
        int has_nan = 0;  // bit 0: a NaN among the taps, bit 1: an infinity
        for (int k = 0; k < kernel_len; ++k) {
            const double v = ty == DSP_F64 ? ((const double*)taps.data())[k] : (double)((const float*)taps.data())[k];
            has_nan |= std::isnan(v) ? 1 : (std::isinf(v) ? 2 : 0);
        }
        const int32_t out_len = out.len > 0 ? out.len : 1;
        const int s_in = m.add_slot(in.len), s_out = m.add_slot(out_len);
        const int io_in = m.add_io(DSP_IO_WF_IN, in.dtype, in.len, in.stride, in.ptr);
        const int io_k = m.add_io(DSP_IO_TAPS, ty, kernel_len, 0, kernel_dev);
        m.add_op(DSP_OP_LOAD, s_in, 0, io_in);
        m.op(DSP_OP_CONVOLVE, s_out, s_in, io_k, {mode, has_nan});
        m.store(s_out, {out.ptr, out_len, out.stride});
        return DSP_OK;
    });
}

int g_moving_window_multi(int ty, const WfIn& in, double length, double num_mw, int32_t mw_type, const WfOut& out, void* st, int64_t* er) {
    return tiny_chain(ty, in.n_wf, st, er, [&](Mini& m) -> int {
        if (floor(num_mw) != num_mw) return dsp_fail(DSP_E_MW_NUM_INT, "%s", dsp_fatal_message(DSP_E_MW_NUM_INT));
        const int s_in = m.add_slot(in.len), s_out = m.add_slot(in.len);
        const int s_tmp = num_mw > 1 ? m.add_slot(in.len) : 0;
        m.load(in, s_in);
        dsp_op& o = m.op(DSP_OP_MOVING_WINDOW_MULTI, s_out, s_in, 0, {mw_type, (int32_t)num_mw, s_tmp});
        o.sp[0] = m.scalar({nullptr, length});
        m.store(s_out, out);
        return DSP_OK;
    });
}

int g_multi_extrema(int ty, const WfIn& in, Cols sp, int32_t direction, void* vt_max, void* vt_min, int32_t out_len, int64_t out_stride,
                    uint32_t* n_max, uint32_t* n_min, void* st, int64_t* er) {
    return tiny_chain(ty, in.n_wf, st, er, [&](Mini& m) {
        m.n_sregs = 2;
        const int s_in = m.add_slot(in.len), s_max = m.add_slot(out_len), s_min = m.add_slot(out_len);
        m.load(in, s_in);
        m.op(DSP_OP_MULTI_EXTREMA, s_max, s_in, 0, {direction, s_min, 0}, sp);
        m.store(s_max, {vt_max, out_len, out_stride});
        m.store(s_min, {vt_min, out_len, out_stride});
        m.store_scalar(0, n_max, DSP_U32);
        m.store_scalar(1, n_min, DSP_U32);
        return DSP_OK;
    });
}

int g_histogram(int ty, const WfIn& in, const WfOut& weights, const WfOut& borders, void* st, int64_t* er) {
    return tiny_chain(ty, in.n_wf, st, er, [&](Mini& m) -> int {
        if (weights.len <= 0 || borders.len <= 0) return dsp_fail(DSP_ERR_ARG, "histogram: weights_out and borders_out hold at least one value");
        const int s_in = m.add_slot(in.len), s_w = m.add_slot(weights.len), s_b = m.add_slot(borders.len);
        m.load(in, s_in);
        m.op(DSP_OP_HISTOGRAM, s_w, s_in, 0, {s_b});
        m.store(s_w, weights);
        m.store(s_b, borders);
        return DSP_OK;
    });
}

int g_histogram_stats(int ty, const WfIn& weights, const WfIn& edges, const Col& max_in, void* mode_out, void* max_out, void* fwhm_out, void* st,
                      int64_t* er) {
    return tiny_chain(ty, weights.n_wf, st, er, [&](Mini& m) -> int {
        if (weights.len <= 0 || edges.len <= 0) return dsp_fail(DSP_ERR_ARG, "histogram_stats: weights_in and edges_in hold at least one value");
        m.n_sregs = 3;
        const int s_w = m.add_slot(weights.len), s_e = m.add_slot(edges.len);
        m.load(weights, s_w);
        m.load(edges, s_e);
        m.op(DSP_OP_HISTOGRAM_STATS, 0, s_w, 0, {s_e, 0}, {max_in});
        int k = 0;
        for (void* out : {mode_out, max_out, fwhm_out}) m.store_scalar(k++, out, ty);
        return DSP_OK;
    });
}

int g_multi_tpt(int ty, const WfIn& in, const void* thr_dev, int32_t n_thr, int64_t thr_stride, const Col& t_start, double polarity, int32_t mode,
                void* t_out, int64_t out_stride, void* st, int64_t* er) {
    if (n_thr == 0) return DSP_OK;  // (no threshold: an empty result)
    return tiny_chain(ty, in.n_wf, st, er, [&](Mini& m) -> int {
        if (n_thr < 0 || !thr_dev) return dsp_fail(DSP_ERR_ARG, "multi_time_point_thresh: a_threshold_dev holds the thresholds on the device");
        const int s_in = m.add_slot(in.len), s_out = m.add_slot(n_thr);
        m.load(in, s_in);
        // the thresholds: a list per row, loaded like rows, or one list for every row, bound like a filter's taps
        int s_thr = -1, io_thr = 0;
        if (thr_stride != 0)
            s_thr = m.load({thr_dev, ty, in.n_wf, n_thr, thr_stride});
        else
            io_thr = m.add_io(DSP_IO_TAPS, ty, n_thr, 0, thr_dev);
        m.op(DSP_OP_MULTI_TIME_POINT_THRESH, s_out, s_in, io_thr, {mode, s_thr}, {t_start, {nullptr, polarity}});
        m.store(s_out, {t_out, n_thr, out_stride});
        return DSP_OK;
    });
}

}  // namespace

extern "C" {

// what every entry point starts and ends with
#define ROWS const void *in, int in_dtype, int64_t n_wf, int32_t wf_len, int64_t in_stride
#define IN WfIn{in, in_dtype, n_wf, wf_len, in_stride}
#define TAIL void *stream, int64_t *err_row
#define TAIL_ARGS stream, err_row

#define DSP_GUFUNCS(SFX, TY, FT) \
    int dsp_bl_subtract_##SFX(ROWS, const FT* baseline_dev, FT baseline, FT* out, int64_t out_stride, TAIL) { \
        return wf2wf(TY, DSP_OP_BL_SUBTRACT, IN, {}, {{baseline_dev, baseline}}, {out, wf_len, out_stride}, TAIL_ARGS); \
    } \
    int dsp_pole_zero_##SFX(ROWS, FT tau, FT* out, int64_t out_stride, TAIL) { \
        return wf2wf(TY, DSP_OP_POLE_ZERO, IN, {}, {{nullptr, tau}}, {out, wf_len, out_stride}, TAIL_ARGS); \
    } \
    int dsp_pole_zero_col_##SFX(ROWS, const FT* tau_dev, FT tau, FT* out, int64_t out_stride, TAIL) { \
        return wf2wf(TY, DSP_OP_POLE_ZERO, IN, {}, {{tau_dev, tau}}, {out, wf_len, out_stride}, TAIL_ARGS); \
    } \
    int dsp_double_pole_zero_col_##SFX(ROWS, const FT* tau1_dev, FT tau1, const FT* tau2_dev, FT tau2, const FT* frac_dev, FT frac, FT* out, \
                                       int64_t out_stride, TAIL) { \
        return wf2wf(TY, DSP_OP_DOUBLE_POLE_ZERO, IN, {}, {{tau1_dev, tau1}, {tau2_dev, tau2}, {frac_dev, frac}}, {out, wf_len, out_stride}, \
                     TAIL_ARGS); \
    } \
    int dsp_double_pole_zero_##SFX(ROWS, FT tau1, FT tau2, FT frac, FT* out, int64_t out_stride, TAIL) { \
        return wf2wf(TY, DSP_OP_DOUBLE_POLE_ZERO, IN, {}, {{nullptr, tau1}, {nullptr, tau2}, {nullptr, frac}}, {out, wf_len, out_stride}, \
                     TAIL_ARGS); \
    } \
    int dsp_trap_filter_##SFX(ROWS, int32_t rise, int32_t flat, FT* out, int64_t out_stride, TAIL) { \
        return wf2wf(TY, DSP_OP_TRAP_FILTER, IN, {rise, flat, 0}, {}, {out, wf_len, out_stride}, TAIL_ARGS); \
    } \
    int dsp_trap_norm_##SFX(ROWS, int32_t rise, int32_t flat, FT* out, int64_t out_stride, TAIL) { \
        return wf2wf(TY, DSP_OP_TRAP_NORM, IN, {rise, flat, 0}, {}, {out, wf_len, out_stride}, TAIL_ARGS); \
    } \
    int dsp_asym_trap_filter_##SFX(ROWS, int32_t rise, int32_t flat, int32_t fall, FT* out, int64_t out_stride, TAIL) { \
        return wf2wf(TY, DSP_OP_ASYM_TRAP, IN, {rise, flat, fall}, {}, {out, wf_len, out_stride}, TAIL_ARGS); \
    } \
    int dsp_fixed_time_pickoff_##SFX(ROWS, const FT* t_in_dev, FT t_in, int32_t mode_char, FT* out, TAIL) { \
        return wf2scalars(TY, DSP_OP_PICKOFF, IN, {mode_char}, {{t_in_dev, t_in}}, {out}, TAIL_ARGS); \
    } \
    int dsp_time_point_thresh_##SFX(ROWS, const FT* threshold_dev, FT threshold, const FT* t_start_dev, FT t_start, FT walk_forward, FT* out, \
                                    TAIL) { \
        return wf2scalars(TY, DSP_OP_TIME_POINT_THRESH, IN, {}, {{threshold_dev, threshold}, {t_start_dev, t_start}, {nullptr, walk_forward}}, \
                          {out}, TAIL_ARGS); \
    } \
    /* time_point_thresh with an interpolation mode, which the op takes as ip[0] */ \
    int dsp_interpolated_time_point_thresh_##SFX(ROWS, const FT* threshold_dev, FT threshold, const FT* t_start_dev, FT t_start, \
                                                 int64_t walk_forward, int32_t mode_char, FT* out, TAIL) { \
        if (mode_char <= 0 || mode_char > 127) return dsp_fail(DSP_ERR_ARG, "interpolated_time_point_thresh: mode must be a character"); \
        return wf2scalars(TY, DSP_OP_INTERP_TIME_POINT_THRESH, IN, {mode_char}, \
                          {{threshold_dev, threshold}, {t_start_dev, t_start}, {nullptr, (double)walk_forward}}, {out}, TAIL_ARGS); \
    } \
    int dsp_min_max_norm_##SFX(ROWS, const FT* a_min_dev, FT a_min, const FT* a_max_dev, FT a_max, FT* out, int64_t out_stride, TAIL) { \
        return g_min_max_norm(TY, IN, {a_min_dev, a_min}, {a_max_dev, a_max}, {out, wf_len, out_stride}, TAIL_ARGS); \
    } \
    int dsp_windower_##SFX(ROWS, const FT* t0_dev, FT t0, FT* out, int32_t out_len, int64_t out_stride, TAIL) { \
        return wf2wf(TY, DSP_OP_WINDOWER, IN, {}, {{t0_dev, t0}}, {out, out_len, out_stride}, TAIL_ARGS); \
    } \
    int dsp_avg_current_##SFX(ROWS, FT length, FT* out, int32_t out_len, int64_t out_stride, TAIL) { \
        return wf2wf(TY, DSP_OP_AVG_CURRENT, IN, {}, {{nullptr, length}}, {out, out_len, out_stride}, TAIL_ARGS); \
    } \
    int dsp_trap_pickoff_##SFX(ROWS, int32_t rise, int32_t flat, const FT* t_pickoff_dev, FT t_pickoff, FT* out, TAIL) { \
        return wf2scalars(TY, DSP_OP_TRAP_WINDOW_PICKOFF, IN, {rise, flat}, {{t_pickoff_dev, t_pickoff}}, {out}, TAIL_ARGS); \
    } \
    int dsp_upsampler_##SFX(ROWS, FT upsample, FT* out, int32_t out_len, int64_t out_stride, TAIL) { \
        return wf2wf(TY, DSP_OP_UPSAMPLER, IN, {}, {{nullptr, upsample}}, {out, out_len, out_stride}, TAIL_ARGS); \
    } \
    int dsp_moving_window_multi_##SFX(ROWS, FT length, FT num_mw, int32_t mw_type, FT* out, int64_t out_stride, TAIL) { \
        return g_moving_window_multi(TY, IN, length, num_mw, mw_type, {out, wf_len, out_stride}, TAIL_ARGS); \
    } \
    int dsp_linear_slope_fit_##SFX(ROWS, FT* mean, FT* stdev, FT* slope, FT* intercept, TAIL) { \
        return wf2scalars(TY, DSP_OP_LINEAR_SLOPE_FIT, IN, {}, {}, {mean, stdev, slope, intercept}, TAIL_ARGS); \
    } \
    int dsp_mean_below_threshold_##SFX(ROWS, const FT* threshold_dev, FT threshold, FT* out, TAIL) { \
        return wf2scalars(TY, DSP_OP_MEAN_BELOW, IN, {}, {{threshold_dev, threshold}}, {out}, TAIL_ARGS); \
    } \
    int dsp_min_max_##SFX(ROWS, FT* t_min, FT* t_max, FT* a_min, FT* a_max, TAIL) { \
        return wf2scalars(TY, DSP_OP_MIN_MAX, IN, {}, {}, {t_min, t_max, a_min, a_max}, TAIL_ARGS); \
    } \
    int dsp_dwt_haar_##SFX(ROWS, int32_t level, int32_t coeff_char, FT* out, int32_t out_len, int64_t out_stride, TAIL) { \
        /* ip[2], the scratch slot = the input slot itself (dead after the transform) */ \
        return wf2wf(TY, DSP_OP_DWT_HAAR, IN, {level, coeff_char, 0}, {}, {out, out_len, out_stride}, TAIL_ARGS); \
    } \
    int dsp_convolve_wf_##SFX(ROWS, const FT* kernel_dev, int32_t kernel_len, int32_t mode_char, FT* out, int32_t out_len, \
                              int64_t out_stride, TAIL) { \
        return g_convolve(TY, IN, kernel_dev, kernel_len, mode_char, {out, out_len, out_stride}, TAIL_ARGS); \
    } \
    int dsp_get_multi_local_extrema_##SFX(ROWS, const FT* a_delta_max_dev, FT a_delta_max, const FT* a_delta_min_dev, FT a_delta_min, \
                                          int32_t search_direction, const FT* a_abs_max_dev, FT a_abs_max, const FT* a_abs_min_dev, \
                                          FT a_abs_min, FT* vt_max_out, FT* vt_min_out, int32_t out_len, int64_t out_stride, \
                                          uint32_t* n_max_out, uint32_t* n_min_out, TAIL) { \
        return g_multi_extrema(TY, IN, \
                               {{a_delta_max_dev, a_delta_max}, {a_delta_min_dev, a_delta_min}, {a_abs_max_dev, a_abs_max}, {a_abs_min_dev, a_abs_min}}, \
                               search_direction, vt_max_out, vt_min_out, out_len, out_stride, n_max_out, n_min_out, TAIL_ARGS); \
    } \
    int dsp_histogram_##SFX(ROWS, FT* weights_out, int32_t n_bins, int64_t weights_stride, FT* borders_out, int32_t borders_len, \
                            int64_t borders_stride, TAIL) { \
        return g_histogram(TY, IN, {weights_out, n_bins, weights_stride}, {borders_out, borders_len, borders_stride}, TAIL_ARGS); \
    } \
    int dsp_histogram_stats_##SFX(const FT* weights_in, int64_t n_wf, int32_t n_bins, int64_t weights_stride, const FT* edges_in, \
                                  int32_t edges_len, int64_t edges_stride, const FT* max_in_dev, FT max_in, FT* mode_out, FT* max_out, \
                                  FT* fwhm_out, TAIL) { \
        return g_histogram_stats(TY, {weights_in, TY, n_wf, n_bins, weights_stride}, {edges_in, TY, n_wf, edges_len, edges_stride}, \
                                 {max_in_dev, max_in}, mode_out, max_out, fwhm_out, TAIL_ARGS); \
    } \
    int dsp_multi_time_point_thresh_##SFX(ROWS, const FT* a_threshold_dev, int32_t n_thresholds, int64_t threshold_stride, \
                                          const FT* t_start_dev, FT t_start, FT polarity, int32_t mode_in, FT* t_out, int64_t out_stride, \
                                          TAIL) { \
        return g_multi_tpt(TY, IN, a_threshold_dev, n_thresholds, threshold_stride, {t_start_dev, t_start}, polarity, mode_in, t_out, \
                           out_stride, TAIL_ARGS); \
    } \
    int dsp_time_over_threshold_##SFX(ROWS, const FT* a_threshold_dev, FT a_threshold, FT* n_samples_out, TAIL) { \
        return wf2scalars(TY, DSP_OP_TIME_OVER_THRESHOLD, IN, {}, {{a_threshold_dev, a_threshold}}, {n_samples_out}, TAIL_ARGS); \
    }

DSP_GUFUNCS(f32, DSP_F32, float)
DSP_GUFUNCS(f64, DSP_F64, double)
#undef DSP_GUFUNCS

// psd and fft: one entry for both loops (compute_dtype), rows of n_bins values -- (re, im) pairs for fft -- out_stride values of the loop's type apart
static int spectrum(int opcode, const WfIn& in, int compute_dtype, void* out, int32_t n_bins, int64_t out_stride, void* st, int64_t* er) {
    const char* name = opcode == DSP_OP_FFT ? "fft" : "psd";
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64) return dsp_fail(DSP_ERR_ARG, "%s: compute_dtype is DSP_F32 or DSP_F64", name);
    if (n_bins < 1 || n_bins > (1 << 19)) return dsp_fail(DSP_ERR_ARG, "%s: the output holds at least one bin", name);
    return wf2wf(compute_dtype, opcode, in, {}, {}, {out, opcode == DSP_OP_FFT ? 2 * n_bins : n_bins, out_stride}, st, er);
}
int dsp_psd(ROWS, int compute_dtype, void* psd_out, int32_t n_bins, int64_t out_stride, TAIL) {
    return spectrum(DSP_OP_PSD, IN, compute_dtype, psd_out, n_bins, out_stride, TAIL_ARGS);
}
int dsp_fft(ROWS, int compute_dtype, void* dft_out, int32_t n_bins, int64_t out_stride, TAIL) {
    return spectrum(DSP_OP_FFT, IN, compute_dtype, dft_out, n_bins, out_stride, TAIL_ARGS);
}
// sort: one entry for both loops too (compute_dtype), rows of wf_len values out_stride values of the loop's type apart
int dsp_sort_rows(ROWS, int compute_dtype, void* sorted_out, int64_t out_stride, TAIL) {
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64) return dsp_fail(DSP_ERR_ARG, "sort: compute_dtype is DSP_F32 or DSP_F64");
    return wf2wf(compute_dtype, DSP_OP_SORT, IN, {}, {}, {sorted_out, wf_len, out_stride}, TAIL_ARGS);
}
// interpolating_upsampler: one entry for both loops too; the ratio is out_len / wf_len, the mode a constant of the call
int dsp_interp_upsample_rows(ROWS, int compute_dtype, int32_t mode, void* out, int32_t out_len, int64_t out_stride, TAIL) {
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64)
        return dsp_fail(DSP_ERR_ARG, "interpolating_upsampler: compute_dtype is DSP_F32 or DSP_F64");
    if (out_len < 1) return dsp_fail(DSP_ERR_ARG, "interpolating_upsampler: the output holds at least one sample (%d given)", out_len);
    return wf2wf(compute_dtype, DSP_OP_INTERP_UPSAMPLE, IN, {mode}, {}, {out, out_len, out_stride}, TAIL_ARGS);
}
// dense_layer_* and, with out_len == 0, classification_layer_*: one entry for both loops; weights and bias are bound like a filter's taps
int dsp_dense_rows(ROWS, int compute_dtype, const void* weights_dev, const void* bias_dev, int32_t activation, void* out, int32_t out_len,
                   int64_t out_stride, TAIL) {
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64) return dsp_fail(DSP_ERR_ARG, "dense_layer: compute_dtype is DSP_F32 or DSP_F64");
    if (out_len < 0 || !weights_dev) return dsp_fail(DSP_ERR_ARG, "dense_layer: weights_dev holds the weights on the device; out_len is m, or 0 for one value per row");
    return tiny_chain(compute_dtype, n_wf, TAIL_ARGS, [&](Mini& m) -> int {
        const int32_t cols = out_len > 0 ? out_len : 1;
        if (wf_len > DSP_DENSE_N_MAX || cols > DSP_DENSE_M_MAX)  // (ahead of the product below)
            return dsp_fail(DSP_ERR_UNSUPPORTED, "dense_layer: " DSP_DENSE_LIMITS_TEXT " (n = %d, m = %d given)", DSP_DENSE_N_MAX, DSP_DENSE_M_MAX, wf_len, cols);
        const int s_in = m.load(IN);
        const int io_w = m.add_io(DSP_IO_TAPS, compute_dtype, wf_len * cols, 0, weights_dev);
        const int io_b = bias_dev ? m.add_io(DSP_IO_TAPS, compute_dtype, cols, 0, bias_dev) : -1;
        if (out_len > 0) {
            const int s_out = m.add_slot(out_len);
            m.op(DSP_OP_DENSE, s_out, s_in, io_w, {activation, io_b, wf_len, out_len});
            m.store(s_out, {out, out_len, out_stride});
        } else {
            m.n_sregs = 1;
            m.op(DSP_OP_DENSE, 0, s_in, io_w, {activation, io_b, wf_len, 0});
            m.store_scalar(0, out, compute_dtype);
        }
        return DSP_OK;
    });
}
// svm_predict: one entry for both loops; the model's five arrays are bound like a filter's taps, float64 in both loops; the decisions are an output
// of the op's own (float64 too), bound only where the caller asks for them
int dsp_svm_rows(ROWS, int compute_dtype, const void* sv_dev, const void* sv_norm_dev, const void* coef_dev, const void* intercept_dev,
                 const void* classes_dev, int32_t n_sv, int32_t n_classes, int32_t kernel_kind, double gamma, void* label_out, void* dec_out,
                 int64_t dec_stride, TAIL) {
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64) return dsp_fail(DSP_ERR_ARG, "svm_predict: compute_dtype is DSP_F32 or DSP_F64");
    if (!sv_dev || !sv_norm_dev || !coef_dev || !intercept_dev || !classes_dev || !label_out)
        return dsp_fail(DSP_ERR_ARG, "svm_predict: the model's five arrays lie on the device as float64; label_out holds a value per row");
    return tiny_chain(compute_dtype, n_wf, TAIL_ARGS, [&](Mini& m) -> int {
        if (wf_len > DSP_DENSE_N_MAX || n_classes > DSP_SVM_CLASSES_MAX)  // (ahead of the products below)
            return dsp_fail(DSP_ERR_UNSUPPORTED, "svm_predict: " DSP_SVM_LIMITS_TEXT " (n = %d, %d classes given)", DSP_DENSE_N_MAX, DSP_SVM_CLASSES_MAX, wf_len, n_classes);
        if (n_classes < 2) return dsp_fail(DSP_ERR_ARG, "svm_predict: a model has at least 2 classes (%d given)", n_classes);
        const int32_t pairs = n_classes * (n_classes - 1) / 2;
        if (n_sv < 1 || wf_len < 1 || (int64_t)n_sv * wf_len > DSP_SVM_MODEL_MAX || (int64_t)n_sv * pairs > DSP_SVM_MODEL_MAX)
            return dsp_fail(DSP_ERR_UNSUPPORTED, "svm_predict: " DSP_SVM_MODEL_TEXT, DSP_SVM_MODEL_MAX, n_sv, wf_len, pairs);
        if (kernel_kind != 0 && kernel_kind != 1) return dsp_fail(DSP_ERR_ARG, "svm_predict: kernel_kind is 0 (rbf) or 1 (linear)");
        if (dec_out && dec_stride < pairs) return dsp_fail(DSP_ERR_ARG, "svm_predict: rows of %d decisions lie at least as many values apart (%lld given)", pairs, (long long)dec_stride);
        const int s_in = m.load(IN);
        const int io_sv = m.add_io(DSP_IO_TAPS, DSP_F64, n_sv * wf_len, 0, sv_dev);
        const int io_norm = m.add_io(DSP_IO_TAPS, DSP_F64, n_sv, 0, sv_norm_dev);
        const int io_coef = m.add_io(DSP_IO_TAPS, DSP_F64, n_sv * pairs, 0, coef_dev);
        const int io_icpt = m.add_io(DSP_IO_TAPS, DSP_F64, pairs, 0, intercept_dev);
        const int io_cls = m.add_io(DSP_IO_TAPS, DSP_F64, n_classes, 0, classes_dev);
        const int io_dec = dec_out ? m.add_io(DSP_IO_WF_OUT, DSP_F64, pairs, dec_stride, dec_out) : -1;
        m.n_sregs = 1;
        m.op(DSP_OP_SVM_PREDICT, 0, s_in, io_sv, {io_norm, io_coef, io_icpt, io_cls}, {{nullptr, gamma}, {nullptr, (double)kernel_kind}, {nullptr, (double)io_dec}});
        m.store_scalar(0, label_out, compute_dtype);
        return DSP_OK;
    });
}
// normalisation_layer: means and variances are bound like a filter's taps; in place in its slot
int dsp_normalisation_rows(ROWS, int compute_dtype, const void* means_dev, const void* variances_dev, void* out, int64_t out_stride, TAIL) {
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64) return dsp_fail(DSP_ERR_ARG, "normalisation_layer: compute_dtype is DSP_F32 or DSP_F64");
    if (!means_dev || !variances_dev) return dsp_fail(DSP_ERR_ARG, "normalisation_layer: means_dev and variances_dev hold len(x_in) values each on the device");
    return tiny_chain(compute_dtype, n_wf, TAIL_ARGS, [&](Mini& m) -> int {
        const int s = m.load(IN);
        const int io_mean = m.add_io(DSP_IO_TAPS, compute_dtype, wf_len, 0, means_dev);
        const int io_var = m.add_io(DSP_IO_TAPS, compute_dtype, wf_len, 0, variances_dev);
        m.op(DSP_OP_NORMALISE, s, s, io_mean, {io_var});
        m.store(s, {out, wf_len, out_stride});
        return DSP_OK;
    });
}
// reflected_convolve_wf: one entry for both loops too; the kernel is bound like convolve_wf's and looked at once here: a NaN among the taps
// makes every row NaN (convolutions.py:160-161)
int dsp_reflected_convolve_rows(ROWS, int compute_dtype, const void* taps_dev, int32_t n_taps, void* out, int64_t out_stride, TAIL) {
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64) return dsp_fail(DSP_ERR_ARG, "reflected_convolve_wf: compute_dtype is DSP_F32 or DSP_F64");
    if (n_taps < 1 || !taps_dev) return dsp_fail(DSP_ERR_ARG, "reflected_convolve_wf: taps_dev holds n_taps >= 1 values of the loop's type on the device");
    return tiny_chain(compute_dtype, n_wf, TAIL_ARGS, [&](Mini& m) -> int {
        if (n_taps > wf_len) return dsp_fail(DSP_ERR_ARG, "The filter is longer than the input waveform (%d taps, %d samples)", n_taps, wf_len);  // (ahead of the read-back)
        const size_t esz = compute_dtype == DSP_F64 ? 8 : 4;
        std::vector<unsigned char> taps(esz * (size_t)n_taps);
        if (int rc = dsp_gufunc_read_back(taps.data(), taps_dev, taps.size())) return rc;
        int has_nan = 0;
        for (int k = 0; k < n_taps; ++k)
            has_nan |= std::isnan(compute_dtype == DSP_F64 ? ((const double*)taps.data())[k] : (double)((const float*)taps.data())[k]) ? 1 : 0;
        const int s_in = m.load(IN), s_out = m.add_slot(wf_len);
        const int io_k = m.add_io(DSP_IO_TAPS, compute_dtype, n_taps, 0, taps_dev);
        m.op(DSP_OP_REFLECTED_CONVOLVE, s_out, s_in, io_k, {has_nan});
        m.store(s_out, {out, wf_len, out_stride});
        return DSP_OK;
    });
}
// rc_cr2 and bi_level_zero_crossing_time_points: one entry each for both loops, like dsp_sort_rows
int dsp_rc_cr2_rows(ROWS, int compute_dtype, double t_tau, void* out, int64_t out_stride, TAIL) {
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64) return dsp_fail(DSP_ERR_ARG, "rc_cr2: compute_dtype is DSP_F32 or DSP_F64");
    return tiny_chain(compute_dtype, n_wf, TAIL_ARGS, [&](Mini& m) -> int {
        const int s_in = m.load(IN), s_out = m.add_slot(wf_len);
        m.op(DSP_OP_RC_CR2, s_out, s_in, 0, {}, {{nullptr, t_tau}});
        m.store(s_out, {out, wf_len, out_stride});
        return DSP_OK;
    });
}
int dsp_bi_level_zero_crossing_rows(ROWS, int compute_dtype, const void* a_pos_threshold_dev, double a_pos_threshold, const void* a_neg_threshold_dev,
                                    double a_neg_threshold, const void* gate_time_dev, double gate_time, const void* t_start_dev, double t_start,
                                    uint32_t* n_crossings_out, void* polarity_out, void* t_trig_times_out, int32_t out_len, int64_t out_stride, TAIL) {
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64)
        return dsp_fail(DSP_ERR_ARG, "bi_level_zero_crossing_time_points: compute_dtype is DSP_F32 or DSP_F64");
    return tiny_chain(compute_dtype, n_wf, TAIL_ARGS, [&](Mini& m) -> int {
        if (out_len < 1) return dsp_fail(DSP_ERR_ARG, "bi_level_zero_crossing_time_points: polarity_out and t_trig_times_out hold at least one entry");
        m.n_sregs = 1;
        const int s_in = m.load(IN), s_pol = m.add_slot(out_len), s_time = m.add_slot(out_len);
        m.op(DSP_OP_BI_LEVEL_ZERO_CROSSING, s_pol, s_in, 0, {s_time, 0},
             {{a_pos_threshold_dev, a_pos_threshold}, {a_neg_threshold_dev, a_neg_threshold}, {gate_time_dev, gate_time}, {t_start_dev, t_start}});
        m.store(s_pol, {polarity_out, out_len, out_stride});
        m.store(s_time, {t_trig_times_out, out_len, out_stride});
        m.store_scalar(0, n_crossings_out, DSP_U32);
        return DSP_OK;
    });
}
// peak_snr_threshold and multi_a_filter: one entry each for both loops; the list is loaded like rows, a list per row
int dsp_peak_snr_threshold_rows(ROWS, int compute_dtype, const void* idx_in_dev, int32_t list_len, int64_t idx_in_stride, const void* ratio_dev, double ratio,
                                double width, void* idx_out, int64_t out_stride, uint32_t* n_idx_out, TAIL) {
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64) return dsp_fail(DSP_ERR_ARG, "peak_snr_threshold: compute_dtype is DSP_F32 or DSP_F64");
    if (list_len == 0) return DSP_OK;  // (no candidate: an empty result)
    return tiny_chain(compute_dtype, n_wf, TAIL_ARGS, [&](Mini& m) -> int {
        if (list_len < 0 || !idx_in_dev) return dsp_fail(DSP_ERR_ARG, "peak_snr_threshold: idx_in_dev holds the candidates on the device");
        m.n_sregs = 1;
        const int s_in = m.load(IN), s_list = m.load({idx_in_dev, compute_dtype, n_wf, list_len, idx_in_stride}), s_out = m.add_slot(list_len);
        m.op(DSP_OP_PEAK_SNR_THRESHOLD, s_out, s_in, 0, {s_list, 0}, {{ratio_dev, ratio}, {nullptr, width}});
        m.store(s_out, {idx_out, list_len, out_stride});
        m.store_scalar(0, n_idx_out, DSP_U32);
        return DSP_OK;
    });
}
int dsp_multi_a_filter_rows(ROWS, int compute_dtype, const void* vt_maxs_in_dev, int32_t list_len, int64_t vt_stride, void* va_max_out, int64_t out_stride, TAIL) {
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64) return dsp_fail(DSP_ERR_ARG, "multi_a_filter: compute_dtype is DSP_F32 or DSP_F64");
    if (list_len == 0) return DSP_OK;  // (no position: an empty result)
    return tiny_chain(compute_dtype, n_wf, TAIL_ARGS, [&](Mini& m) -> int {
        if (list_len < 0 || !vt_maxs_in_dev) return dsp_fail(DSP_ERR_ARG, "multi_a_filter: vt_maxs_in_dev holds the positions on the device");
        const int s_in = m.load(IN), s_list = m.load({vt_maxs_in_dev, compute_dtype, n_wf, list_len, vt_stride}), s_out = m.add_slot(list_len);
        m.op(DSP_OP_MULTI_A_FILTER, s_out, s_in, 0, {s_list});
        m.store(s_out, {va_max_out, list_len, out_stride});
        return DSP_OK;
    });
}
// log_check, poly_fitter, poly_diff / poly_exp_rms: one entry each for both loops; the inverted matrix is bound like a filter's taps, float64 in
// both loops, the coefficients of the residuals are loaded like rows, a row per event
int dsp_log_check_rows(ROWS, int compute_dtype, void* out, int64_t out_stride, TAIL) {
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64) return dsp_fail(DSP_ERR_ARG, "log_check: compute_dtype is DSP_F32 or DSP_F64");
    return wf2wf(compute_dtype, DSP_OP_LOG_CHECK, IN, {}, {}, {out, wf_len, out_stride}, TAIL_ARGS);
}
int dsp_poly_fit_rows(ROWS, int compute_dtype, const double* inv_dev, int32_t n_pars, void* poly_pars_out, int64_t out_stride, TAIL) {
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64) return dsp_fail(DSP_ERR_ARG, "poly_fit: compute_dtype is DSP_F32 or DSP_F64");
    return tiny_chain(compute_dtype, n_wf, TAIL_ARGS, [&](Mini& m) -> int {
        if (n_pars < 1 || !inv_dev) return dsp_fail(DSP_ERR_ARG, "poly_fit: inv_dev holds the n_pars * n_pars >= 1 float64 values of the inverted matrix on the device");
        if (n_pars > DSP_POLY_MAX) return dsp_fail(DSP_ERR_UNSUPPORTED, "poly_fit: " DSP_POLY_MAX_TEXT, DSP_POLY_MAX, n_pars);  // (ahead of the product below)
        const int s_in = m.load(IN), s_out = m.add_slot(n_pars);
        const int io_inv = m.add_io(DSP_IO_TAPS, DSP_F64, n_pars * n_pars, 0, inv_dev);
        m.op(DSP_OP_POLY_FIT, s_out, s_in, io_inv);
        m.store(s_out, {poly_pars_out, n_pars, out_stride});
        return DSP_OK;
    });
}
int dsp_poly_residual_rows(ROWS, int compute_dtype, int32_t exp_rms, const void* poly_pars_dev, int32_t n_pars, int64_t pars_stride, void* mean_out, void* rms_out,
                           TAIL) {
    const char* name = exp_rms ? "poly_exp_rms" : "poly_diff";
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64) return dsp_fail(DSP_ERR_ARG, "%s: compute_dtype is DSP_F32 or DSP_F64", name);
    return tiny_chain(compute_dtype, n_wf, TAIL_ARGS, [&](Mini& m) -> int {
        if (n_pars < 1 || !poly_pars_dev) return dsp_fail(DSP_ERR_ARG, "%s: poly_pars_dev holds n_pars >= 1 coefficients per row on the device", name);
        m.n_sregs = 2;
        const int s_in = m.load(IN), s_pars = m.load({poly_pars_dev, compute_dtype, n_wf, n_pars, pars_stride});
        m.op(exp_rms ? DSP_OP_POLY_EXP_RMS : DSP_OP_POLY_DIFF, 0, s_in, 0, {s_pars});
        m.store_scalar(0, mean_out, compute_dtype);
        m.store_scalar(1, rms_out, compute_dtype);
        return DSP_OK;
    });
}
// inl_correction, get_wf_centroid, wf_alignment, wf_correction: one entry each for both loops; the tables are bound like a filter's taps, in the
// loop's type
int dsp_inl_correction_rows(ROWS, int compute_dtype, const void* inl_dev, int32_t inl_len, void* out, int64_t out_stride, TAIL) {
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64) return dsp_fail(DSP_ERR_ARG, "inl_correction: compute_dtype is DSP_F32 or DSP_F64");
    return tiny_chain(compute_dtype, n_wf, TAIL_ARGS, [&](Mini& m) -> int {
        if (inl_len < 1 || !inl_dev) return dsp_fail(DSP_ERR_ARG, "inl_correction: inl_dev holds the inl_len >= 1 entries of the table on the device");
        const int s_in = m.load(IN), s_out = m.add_slot(wf_len);
        m.op(DSP_OP_INL_CORRECTION, s_out, s_in, m.add_io(DSP_IO_TAPS, compute_dtype, inl_len, 0, inl_dev));
        m.store(s_out, {out, wf_len, out_stride});
        return DSP_OK;
    });
}
int dsp_wf_centroid_rows(ROWS, int compute_dtype, double shift, void* centroid_out, TAIL) {
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64) return dsp_fail(DSP_ERR_ARG, "get_wf_centroid: compute_dtype is DSP_F32 or DSP_F64");
    return tiny_chain(compute_dtype, n_wf, TAIL_ARGS, [&](Mini& m) -> int {
        m.n_sregs = 1;
        const int s_in = m.load(IN);
        m.op(DSP_OP_WF_CENTROID, 0, s_in, 0, {}, {{nullptr, shift}});
        m.store_scalar(0, centroid_out, compute_dtype);
        return DSP_OK;
    });
}
int dsp_wf_alignment_rows(ROWS, int compute_dtype, const void* centroid_dev, double centroid, double shift, double size, void* out, int32_t out_len,
                          int64_t out_stride, TAIL) {
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64) return dsp_fail(DSP_ERR_ARG, "wf_alignment: compute_dtype is DSP_F32 or DSP_F64");
    return tiny_chain(compute_dtype, n_wf, TAIL_ARGS, [&](Mini& m) -> int {
        if (out_len < 1) return dsp_fail(DSP_ERR_ARG, "wf_alignment: w_out holds at least one sample");
        const int s_in = m.load(IN), s_out = m.add_slot(out_len);
        m.op(DSP_OP_WF_ALIGNMENT, s_out, s_in, 0, {}, {{centroid_dev, centroid}, {nullptr, shift}, {nullptr, size}});
        m.store(s_out, {out, out_len, out_stride});
        return DSP_OK;
    });
}
int dsp_wf_correction_rows(ROWS, int compute_dtype, const void* corr_dev, int32_t corr_len, int32_t start_idx, int32_t stop_idx, void* out, int64_t out_stride,
                           TAIL) {
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64) return dsp_fail(DSP_ERR_ARG, "wf_correction: compute_dtype is DSP_F32 or DSP_F64");
    return tiny_chain(compute_dtype, n_wf, TAIL_ARGS, [&](Mini& m) -> int {
        if (corr_len < 1 || !corr_dev) return dsp_fail(DSP_ERR_ARG, "wf_correction: corr_dev holds the corr_len >= 1 entries of w_corr on the device");
        const int s_in = m.load(IN), s_out = m.add_slot(wf_len);
        m.op(DSP_OP_WF_CORRECTION, s_out, s_in, m.add_io(DSP_IO_TAPS, compute_dtype, corr_len, 0, corr_dev), {start_idx, stop_idx});
        m.store(s_out, {out, wf_len, out_stride});
        return DSP_OK;
    });
}
#undef ROWS
#undef IN
#undef TAIL
#undef TAIL_ARGS

}  // extern "C"
