// dsp_plan.cpp -- chain translation without the device: validation, host-evaluated constants, LDS packing by slot lifetime, the shape
// matchers of the specialised kernels and the launch geometry (see dsp_plan.h).  No HIP header, no HIP call: this file is also built for
// the CPU under AddressSanitizer / UBSan and fuzzed (tests/planner_fuzz.cpp).
//
// Reference behaviour mirrored here: constant-only DSPFatal conditions are raised at chain creation with the reference's own
// codes / messages (processors/*.py, cited in include/dspeed_hip.h).
#include "dsp_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

namespace {
thread_local std::string g_last_error;
}

int dsp_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}
void dsp_set_last_error(const char* text) { g_last_error = text ? text : ""; }
const char* dsp_plan_last_error() { return g_last_error.c_str(); }

int dsp_elem_size(int dtype) {
    switch (dtype) {
        case DSP_F32: case DSP_I32: case DSP_U32: return 4;
        case DSP_F64: case DSP_I64: case DSP_U64: return 8;
        case DSP_I16: case DSP_U16: return 2;
        case DSP_BOOL: return 1;
        default: return 0;
    }
}

extern "C" const char* dsp_fatal_message(int code) {
    switch (code) {
        case DSP_E_PZ_NAN: return "Pole-zero filter produced nans in output.";
        case DSP_E_DPZ_SHORT: return "The length of the waveform must be larger than 3 for the filter to work safely";
        case DSP_E_TRAP_RISE: return "The number of samples in the rise section must be positive";
        case DSP_E_TRAP_FLAT: return "The number of samples in the flat section must be positive";
        case DSP_E_TRAP_FALL: return "The number of samples in the fall section must be positive";
        case DSP_E_TRAP_WIDE: return "The trapezoid width is wider than the waveform";
        case DSP_E_FTP_INT: return "fixed_time_pickoff requires integer t_in when using mode 'i'";
        case DSP_E_FTP_MODE: return "Unrecognized interpolation mode";
        case DSP_E_TPT_START_INT: return "The starting index must be an integer";
        case DSP_E_TPT_WALK_INT: return "The search direction must be an integer";
        case DSP_E_TPT_RANGE: return "The starting index is out of range";
        case DSP_E_CONV_LONG: return "The filter is longer than the input waveform";
        case DSP_E_CONV_OUTLEN: return "Output waveform has the wrong length for this convolution mode";
        case DSP_E_CONV_MODE: return "Invalid mode";
        case DSP_E_DWT_LEVEL: return "The level must be a positive integer";
        case DSP_E_DWT_OUTLEN: return "Output waveform has the wrong length for this wavelet level";
        case DSP_E_ZERODIV: return "division by zero";
        case DSP_E_WINDOW_LONG: return "The windowed waveform must be smaller than the input waveform";
        case DSP_E_AVGCUR_RANGE: return "length is out of range, must be between 0 and the length of the waveform";
        case DSP_E_TPO_INT: return "The pick-off index must be an integer";
        case DSP_E_UPSAMPLE: return "Upsample must be greater than 0";
        case DSP_E_MW_LEN_INT: return "The length of the moving window must be an integer";
        case DSP_E_MW_NUM_INT: return "The number of moving windows must be an integer";
        case DSP_E_MW_LEN_RANGE: return "The length of the moving window is out of range";
        case DSP_E_MW_NUM_NEG: return "The number of moving windows much be positive";
        case DSP_E_EXTREMA_LEN: return "The length of your return array must be smaller than the length of your waveform";
        case DSP_E_EXTREMA_DELTA: return "Delta must be positive";
        case DSP_E_EXTREMA_DIR: return "search direction type not found.";
        case DSP_E_HIST_LEN: return "length borders_out must be exactly 1 + length of weights_out";
        case DSP_E_HIST_STATS_LEN: return "length edges_in must be exactly 1 + length of weights_in";
        case DSP_E_MTPT_POLARITY: return "polarity cannot be 0";
        case DSP_E_MTPT_MODE: return "Unrecognized interpolation mode";
        case DSP_E_FFT_LEN: return "Size of fft must be len(w_in)//2+1";  // (raised with the length behind it, as the reference formats it)
        case DSP_E_PSD_LEN: return "Size of psd must be len(w_in)//2+1";
        case DSP_E_RC_CR2_NAN: return "RC-CR^2 filter produced nans in output.";
        case DSP_E_MAF_LEN: return "The length of your return array must be smaller than the length of your waveform";
        case DSP_E_INL_RANGE: return "ADC code out of range for INL array";  // (raised with the code and the table's length, as the reference formats it)
        case DSP_E_ALIGN_CENTROID: return "centroid is nan";
        default: return "";
    }
}

#define fail dsp_fail
#define elem_size dsp_elem_size

// ip[0] of ELEMENTWISE / SCALAR_FUNC: a DSP_FN_* code; the integer loops carry their type (8, 16 or 32 bits; 32 only in the float64 chain,
// whose values hold every 32-bit integer), the float ones nothing
static void note(ChainPlan* ch, const char* fmt, ...) {
    if (!ch->note.empty()) return;  // (the first reason stands)
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    ch->note = buf;
}

struct KernelOnlyRoute;  // (a row of kernel_only_routes, behind the matchers)

// What the passes of dsp_plan_build share: the caller's program, the plan they fill and the tables one pass leaves for the next.
struct PlanCtx {
    const dsp_op* ops;
    int n_ops;
    const dsp_io_desc* io;
    int n_io;
    const int32_t* slot_len;
    int n_slots, n_sregs, compute_dtype;
    ChainPlan* ch;
    bool f64 = false, i64 = false;
    const KernelOnlyRoute* only = nullptr;  // the first route of kernel_only_routes that one of the ops belongs to
    int esz = 4;  // bytes of an LDS element
    // FIR inputs (laid out without the chunk pad); slots that share their LDS region with another
    bool linear[DSP_MAX_SLOTS] = {false}, shares[DSP_MAX_SLOTS] = {false};
    // lifetime (first .. last op of the caller's program that touches the slot) and LDS region [base, base + foot) of every slot
    int first_op[DSP_MAX_SLOTS] = {0}, last_op[DSP_MAX_SLOTS] = {0}, foot[DSP_MAX_SLOTS] = {0}, base[DSP_MAX_SLOTS] = {0};
    std::vector<int> dev_index{};  // caller's op -> position in the device program
    int n_dev_ops = 0;
};

static bool fn_code_ok(int ip0, bool f64, bool i64 = false) {
    const int code = DSP_FN_CODE(ip0), bits = DSP_FN_INT_BITS(ip0);
    if (ip0 < 0 || code > DSP_FN_LAST || (ip0 >> 17) != 0) return false;
    // (64 bits outside an integer program: the float64 chain's waveform loops, exact while results stay below 2^53 -- the caller's promise)
    if (code >= DSP_FN_IADD && code <= DSP_FN_ICAST) return bits == 8 || bits == 16 || (bits == 32 && (f64 || i64)) || (bits == 64 && (i64 || (f64 && code != DSP_FN_ICAST)));
    if (i64) {  // an integer program: no float arithmetic; a comparison may name its loop's type (uint64: unsigned)
        if (code <= DSP_FN_DIV || code == DSP_FN_NEG || code == DSP_FN_FLOORDIV || code >= DSP_FN_RINT) return false;
        return (ip0 >> 8) == 0 || bits == 8 || bits == 16 || bits == 32 || bits == 64;
    }
    return (ip0 >> 8) == 0;
}

// Is the program  LOAD s; [MIN_MAX of s;] [BL_SUBTRACT s <- s;]  POLE_ZERO s <- s;  STORE s  [+ STORE_SCALARs of MIN_MAX's values]  on 16-byte aligned rows
// (dsp_pz.hip)?  The MIN_MAX is that of the rows as they are read: every Ge recipe asks for tp_min / tp_max / wf_min / wf_max of the raw waveform.
static bool match_pz_rows_shape(const PlanCtx& c) {
    ChainPlan* ch = c.ch;
    const dsp_op* ops = c.ops;
    const dsp_io_desc* io = c.io;
    const int32_t* slot_len = c.slot_len;
    int n_ops = c.n_ops;
    const int n_slots = c.n_slots;
    if (c.f64 || n_slots != 1 || n_ops < 3 || n_ops > 9 || ops[0].opcode != DSP_OP_LOAD) return false;
    const dsp_op& ld = ops[0];
    const dsp_io_desc& w = io[ld.io];
    const int len = slot_len[ld.dst];
    if ((w.dtype != DSP_F32 && w.dtype != DSP_I16 && w.dtype != DSP_U16) || ld.ip[0] != 0 || ld.ip[1] != 0 || w.len != len || len % 8 != 0 || len < 8)
        return false;
    const int es = w.dtype == DSP_F32 ? 4 : 2;
    if ((w.row_stride * es) % 16 != 0 || (w.offset * es) % 16 != 0) return false;
    PzArgs& A = ch->pz;
    memset(&A, 0, sizeof A);
    ch->pio_bl = -1;
    for (int k = 0; k < 4; ++k) ch->pio_mm[k] = -1;
    int i = 1, mm_reg = -1;
    if (ops[i].opcode == DSP_OP_MIN_MAX) {  // min_max of the rows as they are read: the kernel streams them anyway
        if (ops[i].src != ld.dst) return false;
        mm_reg = ops[i++].dst;
        A.mm_on = 1;
    }
    // the stores of its four values, wherever they stand behind it
    std::vector<dsp_op> rest(ops, ops + i);
    int pz_at = -1;  // (the pole-zero op's place in the caller's program: its device op holds the constants)
    for (int k = i; k < n_ops; ++k) {
        const dsp_op& o = ops[k];
        if (o.opcode == DSP_OP_POLE_ZERO && pz_at < 0) pz_at = k;
        if (o.opcode != DSP_OP_STORE_SCALAR) {
            rest.push_back(o);
            continue;
        }
        const int which = o.ip[0] - mm_reg;
        if (mm_reg < 0 || which < 0 || which > 3 || ch->pio_mm[which] >= 0 || io[o.io].dtype != DSP_F32) return false;
        ch->pio_mm[which] = o.io;
        A.mm_stride[which] = io[o.io].row_stride;
    }
    if (pz_at < 0 || (int)rest.size() < i + 2) return false;
    ops = rest.data();  // (the program without those stores)
    n_ops = (int)rest.size();
    if (ops[i].opcode == DSP_OP_BL_SUBTRACT) {
        const dsp_op& bs = ops[i++];
        if (bs.dst != ld.dst || bs.src != ld.dst || bs.ip[0] != 0) return false;
        if (bs.sp[0].kind == DSP_ARG_INPUT && io[bs.sp[0].index].dtype == DSP_F32) {
            ch->pio_bl = bs.sp[0].index;
            A.bl_stride = io[ch->pio_bl].row_stride;
        } else if (bs.sp[0].kind == DSP_ARG_CONST) {
            A.bl_const = (float)bs.sp[0].value;
        } else {
            return false;
        }
        A.sub_mode = 1;
    }
    if (i + 2 != n_ops || ops[i].opcode != DSP_OP_POLE_ZERO || ops[i + 1].opcode != DSP_OP_STORE) return false;
    const dsp_op &pz = ops[i], &st = ops[i + 1];
    const bool tau_col = pz.sp[0].kind == DSP_ARG_INPUT && io[pz.sp[0].index].dtype == DSP_F32;
    if (pz.src != ld.dst || pz.dst != ld.dst || (pz.sp[0].kind != DSP_ARG_CONST && !tau_col) || st.src != ld.dst) return false;
    ch->pio_tau = tau_col ? pz.sp[0].index : -1;
    if (tau_col) A.tau_stride = io[ch->pio_tau].row_stride;
    const dsp_io_desc& o = io[st.io];
    if (o.dtype != DSP_F32 || o.len != len || o.row_stride % 4 != 0 || o.offset % 4 != 0) return false;
    const DevOp& dpz = ch->host.ops[c.dev_index[pz_at]];
    A.c = dpz.fc[0];
    A.tau_nan = dpz.ic[0];
    A.wf_stride = w.row_stride;
    A.wf_offset = w.offset;
    A.len = len;
    A.in_kind = w.dtype == DSP_F32 ? 0 : (w.dtype == DSP_I16 ? 1 : 2);
    A.out_stride = o.row_stride;
    ch->pio_wf = ld.io;
    ch->pio_out = st.io;
    return true;
}

// Does the program only read per-event values off rows (dsp_reduce.hip)?
//   LOAD s;  then any of  MIN_MAX of s (once),  AMAX of s (once),  PICKOFF of s at a constant integral time (fixed_time_pickoff, or the plain
//   sample wf[k]; up to DSP_REDUCE_PICKS),  TIME_POINT_THRESH of s from a constant sample or from MIN_MAX's t_min / t_max (up to
//   DSP_REDUCE_WALKS);  then STORE_SCALARs of the registers those made, float32 columns
// The reductions themselves: ops[first ..] on waveform slot `slot` of `len` samples, then the stores; fills A, which the caller has cleared, and
// ch->dio_* (dsp_fir_runs.hip runs the same on the waveform it has just filtered)
static bool match_reduce_ops(ChainPlan* ch, const dsp_op* ops, int first, int n_ops, int slot, int len, const dsp_io_desc* io, ReduceArgs& A) {
    int reg_of_out[5] = {-1, -1, -1, -1, -1}, reg_of_pick[DSP_REDUCE_PICKS] = {-1, -1, -1, -1};
    int reg_of_walk[DSP_REDUCE_WALKS], walk_thr_io[DSP_REDUCE_WALKS], walk_ts_io[DSP_REDUCE_WALKS];
    for (int k = 0; k < DSP_REDUCE_WALKS; ++k) reg_of_walk[k] = walk_thr_io[k] = walk_ts_io[k] = -1;
    // thresholds that are a fraction of a per-event column: SCALAR_AFFINE d <- column * constant + 0 in front of the walk that reads d
    struct Scaled { int reg, io; float factor; };
    std::vector<Scaled> scaled;
    int n_pick = 0, n_walk = 0, i = first;
    for (; i < n_ops; ++i) {
        const dsp_op& o = ops[i];
        if (o.opcode == DSP_OP_MIN_MAX && o.src == slot && reg_of_out[0] < 0) {
            for (int k = 0; k < 4; ++k) reg_of_out[k] = o.dst + k;
        } else if (o.opcode == DSP_OP_AMAX && o.src == slot && reg_of_out[4] < 0) {
            reg_of_out[4] = o.dst;
        } else if (o.opcode == DSP_OP_PICKOFF && o.src == slot && n_pick < DSP_REDUCE_PICKS && o.sp[0].kind == DSP_ARG_CONST && (o.ip[1] == 0 || o.ip[1] == 1)) {
            const double t = (double)(float)o.sp[0].value;
            if (!(t == std::floor(t)) || std::fabs(t) > 1e9) return false;  // (between samples: the interpolating modes stay with the program)
            if (o.ip[1] == 1 && (t < 0 || t >= len)) return false;
            reg_of_pick[n_pick] = o.dst;
            A.pick_at[n_pick] = (t >= 0 && t <= len - 1) ? (int)t : -1;  // fixed_time_pickoff.py:68-74
            A.pick_rule[n_pick] = o.ip[1] == 0;
            ++n_pick;
        } else if (o.opcode == DSP_OP_SCALAR_AFFINE && o.sp[0].kind == DSP_ARG_INPUT && io[o.sp[0].index].dtype == DSP_F32 && o.sp[1].kind == DSP_ARG_CONST &&
                   o.sp[2].kind == DSP_ARG_CONST && o.sp[2].value == 0.0) {
            scaled.push_back({o.dst, o.sp[0].index, (float)o.sp[1].value});
        } else if (o.opcode == DSP_OP_TIME_POINT_THRESH && o.src == slot && n_walk < DSP_REDUCE_WALKS && o.sp[2].kind == DSP_ARG_CONST &&
                   (o.sp[2].value == 0.0 || o.sp[2].value == 1.0)) {
            // threshold: a constant, a float32 column or a fraction of one; start: a constant sample inside the waveform, where MIN_MAX found an
            // extreme (an integer inside the waveform by construction -- the checks of time_point_thresh.py:67-74 cannot fail), a float32
            // column or where an earlier walk of this program ended (checked per event, as the processor does)
            if (o.sp[0].kind == DSP_ARG_INPUT && io[o.sp[0].index].dtype == DSP_F32) {
                walk_thr_io[n_walk] = o.sp[0].index;
                A.walk_thr_stride[n_walk] = io[o.sp[0].index].row_stride;
            } else if (o.sp[0].kind == DSP_ARG_CONST) {
                A.walk_thr_const[n_walk] = (float)o.sp[0].value;
            } else if (o.sp[0].kind == DSP_ARG_REG) {
                const Scaled* sc = nullptr;
                for (const Scaled& c : scaled)
                    if (c.reg == o.sp[0].index) sc = &c;  // (the latest value of the register)
                if (!sc) return false;
                walk_thr_io[n_walk] = sc->io;
                A.walk_thr_stride[n_walk] = io[sc->io].row_stride;
                A.walk_thr_factor[n_walk] = sc->factor;
                A.walk_thr_scaled[n_walk] = 1;
            } else {
                return false;
            }
            int from_walk = -1;
            for (int k = 0; k < n_walk; ++k)
                if (o.sp[1].kind == DSP_ARG_REG && reg_of_walk[k] == o.sp[1].index) from_walk = k;
            if (o.sp[1].kind == DSP_ARG_REG && reg_of_out[0] >= 0 && (o.sp[1].index == reg_of_out[0] || o.sp[1].index == reg_of_out[1])) {
                A.walk_from[n_walk] = o.sp[1].index == reg_of_out[0] ? 1 : 2;
            } else if (o.sp[1].kind == DSP_ARG_CONST) {
                const double t = (double)(float)o.sp[1].value;
                if (!(t == std::floor(t)) || t < 0 || t >= len) return false;
                A.walk_start[n_walk] = (int)t;
            } else if (o.sp[1].kind == DSP_ARG_INPUT && io[o.sp[1].index].dtype == DSP_F32) {
                A.walk_from[n_walk] = 3;
                walk_ts_io[n_walk] = o.sp[1].index;
                A.walk_ts_stride[n_walk] = io[o.sp[1].index].row_stride;
            } else if (from_walk >= 0) {
                A.walk_from[n_walk] = 4 + from_walk;
            } else {
                return false;
            }
            A.walk_forward[n_walk] = o.sp[2].value == 1.0;
            reg_of_walk[n_walk] = o.dst;
            ++n_walk;
        } else {
            break;
        }
    }
    if (i == first || i == n_ops) return false;
    for (int k = 0; k < DSP_REDUCE_WALKS; ++k) {
        ch->dio_walk[k] = -1;
        ch->dio_walk_thr[k] = walk_thr_io[k];
        ch->dio_walk_ts[k] = walk_ts_io[k];
    }
    A.n_walks = n_walk;
    for (const Scaled& c : scaled)  // (a fraction that something other than a walk reads -- a store -- is the program's business)
        for (int j = i; j < n_ops; ++j)
            if (ops[j].opcode == DSP_OP_STORE_SCALAR && ops[j].ip[0] == c.reg) return false;
    for (int k = 0; k < 5; ++k) ch->dio_out[k] = -1;
    for (int k = 0; k < DSP_REDUCE_PICKS; ++k) ch->dio_pick[k] = -1;
    for (; i < n_ops; ++i) {
        const dsp_op& o = ops[i];
        if (o.opcode != DSP_OP_STORE_SCALAR || io[o.io].dtype != DSP_F32) return false;
        bool placed = false;
        for (int k = 0; k < 5 && !placed; ++k)
            if (reg_of_out[k] == o.ip[0] && ch->dio_out[k] < 0) {
                ch->dio_out[k] = o.io;
                A.out_stride[k] = io[o.io].row_stride;
                placed = true;
            }
        for (int k = 0; k < n_pick && !placed; ++k)
            if (reg_of_pick[k] == o.ip[0] && ch->dio_pick[k] < 0) {
                ch->dio_pick[k] = o.io;
                A.pick_stride[k] = io[o.io].row_stride;
                placed = true;
            }
        for (int k = 0; k < n_walk && !placed; ++k)
            if (reg_of_walk[k] == o.ip[0] && ch->dio_walk[k] < 0) {
                ch->dio_walk[k] = o.io;
                A.walk_stride[k] = io[o.io].row_stride;
                placed = true;
            }
        if (!placed) return false;  // (a register stored twice, or one nothing here made)
    }
    for (int k = 0; k < n_walk; ++k) {
        bool feeds = false;
        for (int j = k + 1; j < n_walk; ++j) feeds |= A.walk_from[j] == 4 + k;
        if (ch->dio_walk[k] < 0 && !feeds) return false;  // (a walk nobody stores or starts from: the program's business)
    }
    A.len = len;
    // does anything need the whole row?  The extremes, a pick-off's NaN rule -- or the walks' own NaN rule unless the caller says a row is NaN
    // from its first sample on or not at all (the caller of match_reduce_ops sets need_stream = 1 where it has no such promise)
    A.need_stream = (reg_of_out[0] >= 0 || reg_of_out[4] >= 0 || n_pick > 0) ? 1 : 0;
    return true;
}

static double op_const(const PlanCtx& c, const dsp_op& o, int k);
static bool need_io(const PlanCtx& c, const dsp_op& o, int kind);

// ---- what the matchers of the kernels that stream rows from memory share (dsp_row_stream.h)
constexpr unsigned ROWS_F32_LOOP = 1u << DSP_F32 | 1u << DSP_I16 | 1u << DSP_U16, ROWS_F64 = 1u << DSP_F64, ROWS_F64_LOOP = ROWS_F64 | 1u << DSP_I32 | 1u << DSP_U32;

// The rows such a kernel reads: LOAD `ld` takes them whole, as they lie in memory (nothing screened), and their type is one of `f32_loop` /
// `f64_loop` (bits 1 << DSP_*) for the program's loop.  Fills the block's wf_stride / wf_offset / len and `src`; 16-byte loads where stride,
// offset and length are whole vectors.  `type_why`: the reason from the type test on.
template <typename Args>
static bool bind_rows(const PlanCtx& c, const dsp_op& ld, unsigned f32_loop, unsigned f64_loop, Args& A, RowSource& src, const char** why = nullptr,
                      const char* type_why = nullptr) {
    const dsp_io_desc& w = c.io[ld.io];
    if (ld.ip[0] != 0 || ld.ip[1] != 0 || w.len != c.slot_len[ld.dst]) return false;
    if (why) *why = type_why;
    if (!((c.f64 ? f64_loop : f32_loop) >> w.dtype & 1u)) return false;
    const int64_t es = elem_size(w.dtype);
    A.wf_stride = w.row_stride;
    A.wf_offset = w.offset;
    A.len = w.len;
    src.io = ld.io;
    src.dtype = w.dtype;
    src.vec = (w.row_stride * es) % 16 == 0 && (w.offset * es) % 16 == 0 && (w.len * es) % 16 == 0;
    return true;
}

// ---- the bindings of a kernel-only route.  A pointer of the plan's argument block is bound to a binding of the call here and filled in per
// launch by dsp_internal_plan_fill_args; what nobody binds stays null.  Typed on the member: only a pointer can be bound, and only one of the block.
template <typename T>
static void bind(const PlanCtx& c, T*& member, int io, bool raw = false) {
    ChainPlan* ch = c.ch;
    const ptrdiff_t at = (const char*)&member - (const char*)&ch->only;
    if (at < 0 || at + sizeof member > sizeof ch->only) ch->n_bound = DSP_KERNEL_BINDINGS_MAX;  // (no pointer of the block: refused as an overflow is)
    if (ch->n_bound < DSP_KERNEL_BINDINGS_MAX) ch->bound[ch->n_bound] = {io, (uint16_t)at, raw};  // (io < 0, an operand the op does not have: the pointer stays null)
    ++ch->n_bound;  // (past the capacity: dsp_plan_build refuses the program)
}
// the same for an input whose offset travels in the arguments: the pointer is the binding's as it is handed in
template <typename T>
static void bind_raw(const PlanCtx& c, T*& member, int io) {
    bind(c, member, io, true);
}
template <typename T>
static bool is_bound(const PlanCtx& c, T* const& member) {
    return c.ch->bound_io(member) >= 0;
}
// the rows of a kernel-only route: the one row source of the plan, and the block's wf
template <typename Args>
static bool bind_rows(const PlanCtx& c, const dsp_op& ld, unsigned f32_loop, unsigned f64_loop, Args& A, const char** why, const char* type_why) {
    if (!bind_rows(c, ld, f32_loop, f64_loop, A, c.ch->only_src, why, type_why)) return false;
    bind_raw(c, A.wf, ld.io);
    return true;
}
// The 16-byte stores of a kernel that has them: launch_on_rows' rule for the loads, on the output side.  The plan vouches for the stride
// here, once; the call's pointer for the start (dsp_internal_plan_fill_args).
static void vector_stores(const PlanCtx& c, int32_t& out_vec, void*& out, int64_t out_stride) {
    if ((out_stride * c.esz) % 16 != 0) return;
    c.ch->out_vec_at = (int)((const char*)&out_vec - (const char*)&c.ch->only);
    c.ch->out_ptr_at = (int)((const char*)&out - (const char*)&c.ch->only);
}

// Operand k of `o`, a per-event value: a constant (`value`, as the loop receives it) or a column of the loop's type (`binding`, `stride`)
static bool bind_operand(const PlanCtx& c, const dsp_op& o, int k, int& binding, int64_t& stride, double& value) {
    const dsp_scalar_arg& a = o.sp[k];
    if (a.kind == DSP_ARG_INPUT && c.io[a.index].dtype == c.compute_dtype) {
        binding = a.index;
        stride = c.io[a.index].row_stride;
    } else if (a.kind == DSP_ARG_CONST) {
        value = op_const(c, o, k);
    } else {
        return false;
    }
    return true;
}
// (the column bound to a pointer of the kernel-only block; `raw`: as bind_raw)
template <typename T>
static bool bind_operand(const PlanCtx& c, const dsp_op& o, int k, T*& column, int64_t& stride, double& value, bool raw = false) {
    int binding = -1;
    if (!bind_operand(c, o, k, binding, stride, value)) return false;
    if (binding >= 0) bind(c, column, binding, raw);
    return true;
}

static bool match_reduce_shape(const PlanCtx& c) {
    ChainPlan* ch = c.ch;
    if (c.f64 || c.n_ops < 3 || c.ops[0].opcode != DSP_OP_LOAD) return false;
    const dsp_op& ld = c.ops[0];
    ReduceArgs& A = ch->red;
    memset(&A, 0, sizeof A);
    RowSource src;
    if (!bind_rows(c, ld, ROWS_F32_LOOP, 0, A, src) || !match_reduce_ops(ch, c.ops, 1, c.n_ops, ld.dst, A.len, c.io, A)) return false;
    if (!(ld.ip[2] & 1) && src.dtype == DSP_F32) A.need_stream = 1;  // (float rows without the promise of LOAD ip[2]: a NaN may sit anywhere)
    ch->red_src = src;  // (only now: what a refused shape leaves behind is nobody's)
    return true;
}

// Is the program the peak finder's (dsp_extrema.hip)?
//   LOAD s;  MULTI_EXTREMA of s;  STORE of its two lists;  STORE_SCALAR of its two counts into DSP_U32 columns
// The parameters are constants or columns of the loop's type.  Why not, otherwise: `why` (a program that holds the op runs nowhere else).
static bool match_extrema_shape(const PlanCtx& c, const char** why) {
    ChainPlan* ch = c.ch;
    const dsp_op* ops = c.ops;
    const dsp_io_desc* io = c.io;
    *why = "the program must be exactly LOAD, MULTI_EXTREMA, STORE, STORE, STORE_SCALAR, STORE_SCALAR";
    if (c.n_ops != 6 || c.n_slots != 3 || ops[0].opcode != DSP_OP_LOAD || ops[1].opcode != DSP_OP_MULTI_EXTREMA || ops[2].opcode != DSP_OP_STORE ||
        ops[3].opcode != DSP_OP_STORE || ops[4].opcode != DSP_OP_STORE_SCALAR || ops[5].opcode != DSP_OP_STORE_SCALAR)
        return false;
    const dsp_op &ld = ops[0], &ex = ops[1];
    ExtremaArgs& A = ch->only.ext;
    if (ex.src != ld.dst || !bind_rows(c, ld, ROWS_F32_LOOP, ROWS_F64_LOOP, A, why,
                                       "the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64, int32 or uint32 rows"))
        return false;
    *why = "the two lists are stored once each, the two counts once each into DSP_U32 columns";
    for (int i = 2; i < 4; ++i) {
        const int which = ops[i].src == ex.dst ? 0 : (ops[i].src == ex.ip[1] ? 1 : -1);
        if (which < 0 || is_bound(c, A.vt_out[which])) return false;
        bind(c, A.vt_out[which], ops[i].io);
        A.vt_stride[which] = io[ops[i].io].row_stride;
    }
    for (int i = 4; i < 6; ++i) {
        const int which = ops[i].ip[0] - ex.ip[2];
        if (which < 0 || which > 1 || is_bound(c, A.n_out[which]) || io[ops[i].io].dtype != DSP_U32) return false;
        bind(c, A.n_out[which], ops[i].io);
        A.n_stride[which] = io[ops[i].io].row_stride;
    }
    *why = "a parameter is a constant or a per-event column of the loop's type";
    for (int k = 0; k < 4; ++k)
        if (!bind_operand(c, ex, k, A.par[k], A.par_stride[k], A.par_const[k])) return false;
    A.m = c.slot_len[ex.dst];
    A.direction = ex.ip[0];
    return true;
}

// Is the program one of the histogram kernel's (dsp_hist.hip)?
//   LOAD s;  HISTOGRAM of s;  STORE of its weights and of its borders
//   LOAD s;  HISTOGRAM of s;  HISTOGRAM_STATS of its two slots;  [STORE, STORE;]  STORE_SCALAR of the three registers
//   LOAD weights;  LOAD edges;  HISTOGRAM_STATS of them;  STORE_SCALAR of the three registers
// max_in is a constant or a column of the loop's type.  Why not, otherwise: `why` (a program that holds either op runs nowhere else).
static bool match_hist_shape(const PlanCtx& c, const char** why) {
    ChainPlan* ch = c.ch;
    const dsp_op* ops = c.ops;
    const dsp_io_desc* io = c.io;
    const int n = c.n_ops;
    *why = "the program must be exactly LOAD, HISTOGRAM, STORE, STORE; or LOAD, HISTOGRAM, HISTOGRAM_STATS, [STORE, STORE,] STORE_SCALAR x 3; or "
           "LOAD, LOAD, HISTOGRAM_STATS, STORE_SCALAR x 3";
    auto is = [&](int i, int opcode) { return i < n && ops[i].opcode == opcode; };
    const bool alone = n == 6 && is(0, DSP_OP_LOAD) && is(1, DSP_OP_LOAD) && is(2, DSP_OP_HISTOGRAM_STATS);
    const bool hist = n >= 4 && is(0, DSP_OP_LOAD) && is(1, DSP_OP_HISTOGRAM);
    const bool fused = hist && is(2, DSP_OP_HISTOGRAM_STATS);
    if (!alone && !hist) return false;
    const int n_stores = alone ? 0 : (fused ? n - 6 : 2), first_store = fused ? 3 : 2, first_scalar = alone ? 3 : first_store + n_stores;
    if (c.n_slots != (alone ? 2 : 3) || (n_stores != 0 && n_stores != 2) || n != first_scalar + ((alone || fused) ? 3 : 0)) return false;
    for (int i = first_store; i < first_store + n_stores; ++i)
        if (!is(i, DSP_OP_STORE)) return false;
    for (int i = first_scalar; i < n; ++i)
        if (!is(i, DSP_OP_STORE_SCALAR)) return false;
    HistArgs& A = ch->only.hist;
    const dsp_op* st = nullptr;
    if (alone) {
        st = &ops[2];
        const dsp_op* lw = ops[0].dst == st->src ? &ops[0] : (ops[1].dst == st->src ? &ops[1] : nullptr);
        const dsp_op* le = ops[0].dst == st->ip[0] ? &ops[0] : (ops[1].dst == st->ip[0] ? &ops[1] : nullptr);
        if (!lw || !le || lw == le) return false;
        *why = "histogram_stats alone reads weights and edges as rows of the loop's type";
        for (const dsp_op* l : {lw, le})
            if (l->ip[0] != 0 || l->ip[1] != 0 || io[l->io].dtype != c.compute_dtype) return false;
        bind_raw(c, A.w_in, lw->io);
        bind_raw(c, A.e_in, le->io);
        A.w_in_stride = io[lw->io].row_stride;
        A.w_in_offset = io[lw->io].offset;
        A.e_in_stride = io[le->io].row_stride;
        A.e_in_offset = io[le->io].offset;
        A.m = c.slot_len[st->src];
        ch->only_src.dtype = c.compute_dtype;
    } else {
        const dsp_op &ld = ops[0], &hi = ops[1];
        if (hi.src != ld.dst || !bind_rows(c, ld, ROWS_F32_LOOP, ROWS_F64, A, why,
                                           "the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"))
            return false;
        *why = "histogram_stats in the same program reads exactly the histogram's weights and borders";
        if (fused) {
            st = &ops[2];
            if (st->src != hi.dst || st->ip[0] != hi.ip[0]) return false;
        }
        *why = "the weights and the borders are stored once each";
        for (int i = first_store; i < first_store + n_stores; ++i) {
            void*& out = ops[i].src == hi.dst ? A.w_out : A.b_out;
            if ((ops[i].src != hi.dst && ops[i].src != hi.ip[0]) || is_bound(c, out)) return false;
            bind(c, out, ops[i].io);
            (ops[i].src == hi.dst ? A.w_stride : A.b_stride) = io[ops[i].io].row_stride;
        }
        A.m = c.slot_len[hi.dst];
        A.max_blocks = hi.ip[1];
    }
    if (st) {
        *why = "mode_out, max_out and fwhm_out are stored once each, in the loop's type";
        for (int i = first_scalar; i < n; ++i) {
            const int which = ops[i].ip[0] - st->ip[1];
            if (which < 0 || which > 2 || is_bound(c, A.s_out[which]) || io[ops[i].io].dtype != c.compute_dtype) return false;
            bind(c, A.s_out[which], ops[i].io);
            A.s_stride[which] = io[ops[i].io].row_stride;
        }
        *why = "max_in is a constant or a per-event column of the loop's type";
        if (!bind_operand(c, *st, 0, A.max_in, A.max_in_stride, A.max_in_const)) return false;
        A.stats = 1;
    }
    return true;
}

// Is the program one of the threshold kernel's (dsp_thresh.hip)?
//   LOAD s;  MULTI_TIME_POINT_THRESH of s, its thresholds one list for every row (the op's DSP_IO_TAPS binding);  STORE of t_out
//   LOAD s;  LOAD of the thresholds, a list per row;  MULTI_TIME_POINT_THRESH of s and of them;  STORE of t_out
//   LOAD s;  TIME_OVER_THRESHOLD of s;  STORE_SCALAR of its register
// t_start and time_over_threshold's threshold are constants or columns of the loop's type.  Why not, otherwise: `why`.
static bool match_thresh_shape(const PlanCtx& c, const char** why) {
    ChainPlan* ch = c.ch;
    const dsp_op* ops = c.ops;
    const dsp_io_desc* io = c.io;
    const int n = c.n_ops;
    *why = "the program must be exactly LOAD, [LOAD of the thresholds,] MULTI_TIME_POINT_THRESH, STORE; or LOAD, TIME_OVER_THRESHOLD, STORE_SCALAR";
    auto is = [&](int i, int opcode) { return i < n && ops[i].opcode == opcode; };
    const bool tot = n == 3 && c.n_slots == 1 && is(0, DSP_OP_LOAD) && is(1, DSP_OP_TIME_OVER_THRESHOLD) && is(2, DSP_OP_STORE_SCALAR);
    const bool one_list = n == 3 && c.n_slots == 2 && is(0, DSP_OP_LOAD) && is(1, DSP_OP_MULTI_TIME_POINT_THRESH) && is(2, DSP_OP_STORE);
    const bool lists = n == 4 && c.n_slots == 3 && is(0, DSP_OP_LOAD) && is(1, DSP_OP_LOAD) && is(2, DSP_OP_MULTI_TIME_POINT_THRESH) && is(3, DSP_OP_STORE);
    if (!tot && !one_list && !lists) return false;
    const dsp_op& op = ops[lists ? 2 : 1];
    const dsp_op* ld = ops[0].dst == op.src ? &ops[0] : (lists && ops[1].dst == op.src ? &ops[1] : nullptr);
    ThreshArgs& A = ch->only.thresh;
    if (!ld || !bind_rows(c, *ld, ROWS_F32_LOOP, ROWS_F64, A, why,
                          "the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"))
        return false;
    const dsp_op& st = ops[n - 1];
    if (tot) {
        *why = "the threshold is a constant or a per-event column of the loop's type; the count is stored once, in the loop's type";
        // (raw, as the lists below: A.thr is one pointer for both ops, and the kernel reads time_over_threshold's column from it as it is handed in)
        if (!bind_operand(c, op, 0, A.thr, A.thr_stride, A.thr_const, true) || st.ip[0] != op.dst || io[st.io].dtype != c.compute_dtype) return false;
        A.m = 0;
    } else {
        *why = "the thresholds are one list for every row (the op's DSP_IO_TAPS binding, ip[1] < 0) or a list per row, loaded into slot ip[1], in the loop's type";
        if (lists) {
            const dsp_op* lt = ld == &ops[0] ? &ops[1] : &ops[0];
            if (op.ip[1] != lt->dst || lt->dst == op.src || lt->ip[0] != 0 || lt->ip[1] != 0 || io[lt->io].dtype != c.compute_dtype) return false;
            bind_raw(c, A.thr, lt->io);
            A.thr_stride = io[lt->io].row_stride;
            A.thr_offset = io[lt->io].offset;
        } else {
            if (op.ip[1] >= 0 || !need_io(c, op, DSP_IO_TAPS) || io[op.io].len != c.slot_len[op.dst]) return false;
            bind_raw(c, A.thr, op.io);
            A.thr_stride = 0;
            A.thr_offset = io[op.io].offset;
        }
        *why = "t_start is a constant or a per-event column of the loop's type; t_out is stored once, in the loop's type";
        if (!bind_operand(c, op, 0, A.ts, A.ts_stride, A.ts_const) || st.src != op.dst || io[st.io].dtype != c.compute_dtype) return false;
        A.m = c.slot_len[op.dst];
        A.polarity = op_const(c, op, 1) > 0 ? 1 : -1;
        A.mode = op.ip[0];
    }
    bind(c, A.out, st.io);
    A.out_stride = io[st.io].row_stride;
    return true;
}

// Is the program one of the spectrum kernel's (dsp_spectrum.hip)?
//   LOAD s;  PSD of s;  STORE of its n / 2 + 1 bins
//   LOAD s;  FFT of s;  STORE of its 2 (n / 2 + 1) values, (re, im) pairs
// Lengths and limits are lower_op's business (every program that holds either op passes there first).  Why not, otherwise: `why`.
static bool match_spectrum_shape(const PlanCtx& c, const char** why) {
    ChainPlan* ch = c.ch;
    const dsp_op* ops = c.ops;
    *why = "the program must be exactly LOAD, PSD, STORE or LOAD, FFT, STORE";
    if (c.n_ops != 3 || c.n_slots != 2 || ops[0].opcode != DSP_OP_LOAD || (ops[1].opcode != DSP_OP_PSD && ops[1].opcode != DSP_OP_FFT) ||
        ops[2].opcode != DSP_OP_STORE)
        return false;
    const dsp_op &ld = ops[0], &op = ops[1], &st = ops[2];
    SpectrumArgs& A = ch->only.spec;
    if (op.src != ld.dst || !bind_rows(c, ld, ROWS_F32_LOOP, ROWS_F64, A, why,
                                       "the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"))
        return false;
    *why = "the spectrum is stored once, in the loop's type";
    if (st.src != op.dst || c.io[st.io].dtype != c.compute_dtype) return false;
    A.m = A.len / 2 + 1;
    A.complex_out = op.opcode == DSP_OP_FFT ? 1 : 0;
    A.points = dsp_spectrum::points(A.len);
    for (A.log2_points = 0; (1 << A.log2_points) < A.points; ++A.log2_points) {}
    A.bluestein = dsp_spectrum::pow2(A.len) ? 0 : 1;
    A.wide = dsp_spectrum::wide(A.len, c.esz) ? 1 : 0;
    bind(c, A.out, st.io);
    A.out_stride = c.io[st.io].row_stride;
    return true;
}

// Is the program the sorting kernel's (dsp_sort.hip)?
//   LOAD s;  SORT of s;  STORE of its n samples
// Lengths and limits are lower_op's business (every program that holds the op passes there first).  Why not, otherwise: `why`.
static bool match_sort_shape(const PlanCtx& c, const char** why) {
    ChainPlan* ch = c.ch;
    const dsp_op* ops = c.ops;
    *why = "the program must be exactly LOAD, SORT, STORE";
    if (c.n_ops != 3 || c.n_slots != 2 || ops[0].opcode != DSP_OP_LOAD || ops[1].opcode != DSP_OP_SORT || ops[2].opcode != DSP_OP_STORE) return false;
    const dsp_op &ld = ops[0], &op = ops[1], &st = ops[2];
    SortArgs& A = ch->only.sort;
    if (op.src != ld.dst || !bind_rows(c, ld, ROWS_F32_LOOP, ROWS_F64, A, why,
                                       "the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"))
        return false;
    *why = "the sorted row is stored once, whole, in the loop's type";
    const dsp_io_desc& o = c.io[st.io];
    if (st.src != op.dst || o.dtype != c.compute_dtype || o.len != A.len) return false;
    A.padded = dsp_sort::padded(A.len);
    A.wide = dsp_sort::wide(A.len) ? 1 : 0;
    bind(c, A.out, st.io);
    A.out_stride = o.row_stride;
    return true;
}

// Is the program the resampling kernel's (dsp_interp.hip)?
//   LOAD s;  INTERP_UPSAMPLE of s into a slot of m samples;  STORE of its m samples
// Mode, lengths and limits are lower_op's business (every program that holds the op passes there first).  Why not, otherwise: `why`.
static bool match_interp_shape(const PlanCtx& c, const char** why) {
    ChainPlan* ch = c.ch;
    const dsp_op* ops = c.ops;
    *why = "the program must be exactly LOAD, INTERP_UPSAMPLE, STORE";
    if (c.n_ops != 3 || c.n_slots != 2 || ops[0].opcode != DSP_OP_LOAD || ops[1].opcode != DSP_OP_INTERP_UPSAMPLE || ops[2].opcode != DSP_OP_STORE)
        return false;
    const dsp_op &ld = ops[0], &op = ops[1], &st = ops[2];
    InterpArgs& A = ch->only.interp;
    if (op.src != ld.dst || !bind_rows(c, ld, ROWS_F32_LOOP, ROWS_F64, A, why,
                                       "the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"))
        return false;
    *why = "the resampled row is stored once, whole, in the loop's type";
    const dsp_io_desc& o = c.io[st.io];
    if (st.src != op.dst || o.dtype != c.compute_dtype || o.len != c.slot_len[op.dst]) return false;
    A.out_len = o.len;
    A.mode = op.ip[0];
    A.wide = dsp_interp::wide(A.mode, A.len, c.esz) ? 1 : 0;
    bind(c, A.out, st.io);
    A.out_stride = o.row_stride;
    vector_stores(c, A.out_vec, A.out, A.out_stride);
    return true;
}

// Is the program one of the dense-layer kernel's (dsp_dense.hip)?
//   LOAD s;  [NORMALISE of s, in place;]  DENSE of s into a slot of m samples;  STORE of its m samples
//   LOAD s;  [NORMALISE of s, in place;]  DENSE of s into a scalar register (the classification form);  STORE_SCALAR of it
//   LOAD s;  NORMALISE of s, in place;  STORE of its n samples
// Operands and limits are lower_op's business (every program that holds either op passes there first).  Why not, otherwise: `why`.
static bool match_dense_shape(const PlanCtx& c, const char** why) {
    ChainPlan* ch = c.ch;
    const dsp_op* ops = c.ops;
    const int n = c.n_ops;
    *why = "the program must be exactly LOAD, [NORMALISE,] DENSE, STORE; LOAD, [NORMALISE,] DENSE, STORE_SCALAR; or LOAD, NORMALISE, STORE";
    auto is = [&](int i, int opcode) { return i < n && ops[i].opcode == opcode; };
    if (n < 3 || n > 4 || !is(0, DSP_OP_LOAD)) return false;
    const dsp_op* norm = is(1, DSP_OP_NORMALISE) ? &ops[1] : nullptr;
    const dsp_op* dense = is(norm ? 2 : 1, DSP_OP_DENSE) ? &ops[norm ? 2 : 1] : nullptr;
    const dsp_op& st = ops[n - 1];
    if (n != 2 + (norm ? 1 : 0) + (dense ? 1 : 0)) return false;
    const bool classify = dense && dense->ip[3] == 0;
    if (st.opcode != (classify ? DSP_OP_STORE_SCALAR : DSP_OP_STORE) || c.n_slots != (dense && !classify ? 2 : 1)) return false;
    const dsp_op& ld = ops[0];
    DenseArgs& A = ch->only.dense;
    if ((norm && norm->src != ld.dst) || (dense && dense->src != ld.dst) ||
        !bind_rows(c, ld, ROWS_F32_LOOP, ROWS_F64, A, why, "the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"))
        return false;
    *why = "the result is stored once, whole, in the loop's type";
    const dsp_io_desc& o = c.io[st.io];
    if (o.dtype != c.compute_dtype) return false;
    if (classify ? st.ip[0] != dense->dst : (st.src != (dense ? dense->dst : ld.dst) || o.len != (dense ? dense->ip[3] : A.len))) return false;
    if (norm) {
        A.normalise = 1;
        bind(c, A.means, norm->io);
        bind(c, A.variances, norm->ip[0]);
    }
    if (dense) {
        A.m = classify ? 1 : dense->ip[3];
        A.activation = dense->ip[0];
        bind(c, A.weights, dense->io);
        bind(c, A.bias, dense->ip[1]);
    }
    bind(c, A.out, st.io);
    A.out_stride = o.row_stride;
    return true;
}

// Is the program the support-vector classifier's (dsp_svm.hip)?
//   LOAD s;  SVM_PREDICT of s into a scalar register;  STORE_SCALAR of it
// The model's bindings and the limits are lower_op's business (every program that holds the op passes there first).  Why not, otherwise: `why`.
static bool match_svm_shape(const PlanCtx& c, const char** why) {
    ChainPlan* ch = c.ch;
    const dsp_op* ops = c.ops;
    *why = "the program must be exactly LOAD, SVM_PREDICT, STORE_SCALAR";
    if (c.n_ops != 3 || c.n_slots != 1 || ops[0].opcode != DSP_OP_LOAD || ops[1].opcode != DSP_OP_SVM_PREDICT || ops[2].opcode != DSP_OP_STORE_SCALAR) return false;
    const dsp_op &ld = ops[0], &op = ops[1], &st = ops[2];
    SvmArgs& A = ch->only.svm;
    if (op.src != ld.dst || !bind_rows(c, ld, 1u << DSP_F32, ROWS_F64 | 1u << DSP_F32, A, why,
                                       "the float32 loop takes float32 rows, the float64 loop float32 or float64 rows"))
        return false;
    *why = "the label is stored once, in the loop's type";
    const dsp_io_desc& o = c.io[st.io];
    if (st.ip[0] != op.dst || o.dtype != c.compute_dtype) return false;
    A.n_sv = c.io[op.ip[0]].len;
    A.n_classes = c.io[op.ip[3]].len;
    A.n_pairs = c.io[op.ip[2]].len;
    A.linear = op.sp[1].value != 0.0 ? 1 : 0;
    A.f64 = c.f64 ? 1 : 0;
    A.gamma = op.sp[0].value;
    A.label_stride = o.row_stride;
    bind(c, A.sv, op.io);
    bind(c, A.sv_norm, op.ip[0]);
    bind(c, A.coef, op.ip[1]);
    bind(c, A.intercept, op.ip[2]);
    bind(c, A.classes, op.ip[3]);
    bind(c, A.label, st.io);
    const int dec = (int)op.sp[2].value;
    bind(c, A.dec, dec);
    if (dec >= 0) A.dec_stride = c.io[dec].row_stride;
    return true;
}

// Is the program one of the mirrored-edge FIR kernel's (dsp_reflect.hip)?
//   LOAD s;  REFLECTED_CONVOLVE of s into a slot of as many samples;  STORE of them
//   LOAD s;  REFLECTED_CONVOLVE of s;  AVG_CURRENT of the filtered row (a constant length);  STORE of the current [and of the filtered row]
// Taps, lengths and limits are lower_op's business (every program that holds the op passes there first).  Why not, otherwise: `why`.
static bool match_reflect_shape(const PlanCtx& c, const char** why) {
    ChainPlan* ch = c.ch;
    const dsp_op* ops = c.ops;
    const int n = c.n_ops;
    *why = "the program must be exactly LOAD, REFLECTED_CONVOLVE, STORE; or LOAD, REFLECTED_CONVOLVE, AVG_CURRENT, STORE [, STORE]";
    auto is = [&](int i, int opcode) { return i < n && ops[i].opcode == opcode; };
    if (n < 3 || !is(0, DSP_OP_LOAD) || !is(1, DSP_OP_REFLECTED_CONVOLVE)) return false;
    const bool fused = is(2, DSP_OP_AVG_CURRENT);
    const int first_store = fused ? 3 : 2, n_stores = n - first_store;
    if (n_stores < 1 || n_stores > (fused ? 2 : 1) || c.n_slots != (fused ? 3 : 2)) return false;
    for (int i = first_store; i < n; ++i)
        if (!is(i, DSP_OP_STORE)) return false;
    const dsp_op &ld = ops[0], &op = ops[1];
    ReflectArgs& A = ch->only.reflect;
    if (op.src != ld.dst || !bind_rows(c, ld, ROWS_F32_LOOP, ROWS_F64, A, why,
                                       "the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"))
        return false;
    if (fused) {
        const dsp_op& ac = ops[2];
        *why = "the avg_current in the same program reads exactly the filtered row, with a constant length";
        int binding = -1;
        int64_t stride = 0;
        if (ac.src != op.dst || ac.dst == op.dst || ac.dst == ld.dst || !bind_operand(c, ac, 0, binding, stride, A.length) || binding >= 0) return false;
        A.lag = (int)A.length;  // (0 < lag < n, and the current's slot holds n - lag samples: lower_op's DSP_OP_AVG_CURRENT)
    }
    *why = fused ? "the current is stored once, whole, in the loop's type, and the filtered row at most once" : "the filtered row is stored once, whole, in the loop's type";
    for (int i = first_store; i < n; ++i) {
        const dsp_op& st = ops[i];
        const dsp_io_desc& o = c.io[st.io];
        const bool current = fused && st.src == ops[2].dst;
        void*& out = current ? A.cur : A.out;
        if ((!current && st.src != op.dst) || is_bound(c, out) || o.dtype != c.compute_dtype || o.len != c.slot_len[st.src]) return false;
        bind(c, out, st.io);
        (current ? A.cur_stride : A.out_stride) = o.row_stride;
    }
    if (fused && !is_bound(c, A.cur)) return false;
    A.n_taps = c.io[op.io].len;
    A.taps_nan = op.ip[0] & 1;
    A.wide = dsp_reflect::wide(A.len, A.n_taps, c.esz) ? 1 : 0;
    bind(c, A.taps, op.io);
    vector_stores(c, A.out_vec, A.out, A.out_stride);
    return true;
}

// Is the program one of the pile-up kernel's (dsp_pileup.hip)?
//   LOAD s;  RC_CR2 of s into a slot of as many samples;  STORE of them
//   LOAD s;  BI_LEVEL_ZERO_CROSSING of s;  STORE of its two lists;  STORE_SCALAR of its count into a DSP_U32 column
//   LOAD s;  RC_CR2 of s;  BI_LEVEL_ZERO_CROSSING of the filtered row;  [STORE of the filtered row;]  STORE, STORE;  STORE_SCALAR
// each with or without  BL_SUBTRACT s <- s  (bl_subtract.py, a constant or a column of the loop's type) behind the LOAD: done as the rows are read.
// The walk's operands are constants or columns of the loop's type; t_tau, lengths and limits are lower_op's business (every program that holds
// either op passes there first).  Why not, otherwise: `why`.
static bool match_pileup_shape(const PlanCtx& c, const char** why) {
    ChainPlan* ch = c.ch;
    const dsp_op* ops = c.ops;
    const dsp_io_desc* io = c.io;
    const int n = c.n_ops;
    *why = "the program must be exactly LOAD, RC_CR2, STORE; or LOAD, BI_LEVEL_ZERO_CROSSING, STORE, STORE, STORE_SCALAR; or LOAD, RC_CR2, "
           "BI_LEVEL_ZERO_CROSSING, [STORE of the filtered row,] STORE, STORE, STORE_SCALAR (a BL_SUBTRACT of the rows, in place, may follow the LOAD)";
    auto is = [&](int i, int opcode) { return i >= 0 && i < n && ops[i].opcode == opcode; };
    if (n < 3 || !is(0, DSP_OP_LOAD)) return false;
    const int first = is(1, DSP_OP_BL_SUBTRACT) ? 2 : 1;
    const bool filter = is(first, DSP_OP_RC_CR2), walk = is(filter ? first + 1 : first, DSP_OP_BI_LEVEL_ZERO_CROSSING);
    if (!filter && !walk) return false;
    const int first_store = first + (filter ? 1 : 0) + (walk ? 1 : 0);
    const int n_stores = walk ? n - 1 - first_store : n - first_store;  // (behind them the walk's STORE_SCALAR)
    if (c.n_slots != 1 + (filter ? 1 : 0) + (walk ? 2 : 0) || (walk ? (n_stores != 2 && !(filter && n_stores == 3)) || !is(n - 1, DSP_OP_STORE_SCALAR) : n_stores != 1))
        return false;
    for (int i = first_store; i < first_store + n_stores; ++i)
        if (!is(i, DSP_OP_STORE)) return false;
    const dsp_op& ld = ops[0];
    const dsp_op* fi = filter ? &ops[first] : nullptr;
    const dsp_op* wk = walk ? &ops[filter ? first + 1 : first] : nullptr;
    PileupArgs& A = ch->only.pileup;
    if ((fi ? fi->src : wk->src) != ld.dst || !bind_rows(c, ld, ROWS_F32_LOOP, ROWS_F64, A, why,
                                                        "the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"))
        return false;
    if (first == 2) {
        const dsp_op& bs = ops[1];
        *why = "the BL_SUBTRACT behind the LOAD works on the rows in place (bl_subtract, ip[0] = 0), its baseline a constant or a per-event column of the loop's type";
        if (bs.dst != ld.dst || bs.src != ld.dst || bs.ip[0] != 0 || !bind_operand(c, bs, 0, A.sub, A.sub_stride, A.sub_const)) return false;
        A.sub_mode = 1;
    }
    *why = "the walk in the same program reads exactly the filtered row";
    if (fi && wk && (wk->src != fi->dst || wk->dst == ld.dst || wk->ip[0] == ld.dst)) return false;
    *why = "the filtered row and the two lists are stored once each, whole, in the loop's type; the count once, into a DSP_U32 column";
    for (int i = first_store; i < first_store + n_stores; ++i) {
        const dsp_op& st = ops[i];
        const dsp_io_desc& o = io[st.io];
        void** out = fi && st.src == fi->dst ? &A.out : (wk && st.src == wk->dst ? &A.list[0] : (wk && st.src == wk->ip[0] ? &A.list[1] : nullptr));
        if (!out || is_bound(c, *out) || o.dtype != c.compute_dtype || o.len != c.slot_len[st.src]) return false;
        bind(c, *out, st.io);
        if (out == &A.out) A.out_stride = o.row_stride;
        else A.list_stride[out == &A.list[0] ? 0 : 1] = o.row_stride;
    }
    if (wk) {
        const dsp_op& sc = ops[n - 1];
        const int list0 = ch->bound_io(A.list[0]), list1 = ch->bound_io(A.list[1]), row = ch->bound_io(A.out);
        if (list0 < 0 || list1 < 0 || list0 == list1 || list0 == row || list1 == row ||
            sc.ip[0] != wk->ip[1] || io[sc.io].dtype != DSP_U32)  // (every output its own binding)
            return false;
        bind(c, A.n_out, sc.io);
        A.n_stride = io[sc.io].row_stride;
        *why = "a threshold, the gate and t_start are constants or per-event columns of the loop's type";
        for (int k = 0; k < 4; ++k)
            if (!bind_operand(c, *wk, k, A.par[k], A.par_stride[k], A.par_const[k])) return false;
        A.m = c.slot_len[wk->dst];
    } else if (!is_bound(c, A.out)) {
        return false;
    }
    if (fi) {  // rc_cr2.py:66-71 with numba's typing: -1 / t_tau in float64 whatever the loop, the powers as products
        const double tau = op_const(c, *fi, 0), a = exp(-1.0 / tau);
        A.c1 = 3.0 * a;
        A.c2 = 3.0 * (a * a);
        A.c3 = a * (a * a);
        A.tau_nan = std::isnan(tau) ? 1 : 0;
    }
    A.filter = fi ? 1 : 0;
    A.walk = wk ? 1 : 0;
    vector_stores(c, A.out_vec, A.out, A.out_stride);
    return true;
}

// Is the program one of the pulse picker's (dsp_pulses.hip)?
//   LOAD s;  LOAD of the candidates, a list per row;  PEAK_SNR_THRESHOLD of s and of them;  STORE of idx_out;  STORE_SCALAR of the count (DSP_U32)
//   LOAD s;  LOAD of the positions;  MULTI_A_FILTER of s and of them;  STORE of va_max_out
//   LOAD s;  LOAD of the candidates;  PEAK_SNR_THRESHOLD;  MULTI_A_FILTER of s at idx_out;  [STORE of idx_out;]  STORE of va_max_out;  STORE_SCALAR
// ratio_in is a constant or a column of the loop's type; the width, the lists' lengths and the limits are lower_op's business (every program
// that holds either op passes there first).  Why not, otherwise: `why`.
static bool match_pulses_shape(const PlanCtx& c, const char** why) {
    ChainPlan* ch = c.ch;
    const dsp_op* ops = c.ops;
    const dsp_io_desc* io = c.io;
    const int n = c.n_ops;
    *why = "the program must be exactly LOAD, LOAD of the list, PEAK_SNR_THRESHOLD, STORE, STORE_SCALAR; or LOAD, LOAD of the list, MULTI_A_FILTER, STORE; or LOAD, "
           "LOAD of the list, PEAK_SNR_THRESHOLD, MULTI_A_FILTER, [STORE of idx_out,] STORE of va_max_out, STORE_SCALAR";
    auto is = [&](int i, int opcode) { return i >= 0 && i < n && ops[i].opcode == opcode; };
    if (n < 4 || !is(0, DSP_OP_LOAD) || !is(1, DSP_OP_LOAD)) return false;
    const bool pick = is(2, DSP_OP_PEAK_SNR_THRESHOLD), amp = is(pick ? 3 : 2, DSP_OP_MULTI_A_FILTER);
    if (!pick && !amp) return false;
    const int first_store = 2 + (pick ? 1 : 0) + (amp ? 1 : 0);
    const int n_stores = pick ? n - 1 - first_store : n - first_store;  // (behind them the picker's STORE_SCALAR)
    if (c.n_slots != 2 + (pick ? 1 : 0) + (amp ? 1 : 0) || (pick && !is(n - 1, DSP_OP_STORE_SCALAR)) || (pick && amp ? n_stores != 1 && n_stores != 2 : n_stores != 1))
        return false;
    for (int i = first_store; i < first_store + n_stores; ++i)
        if (!is(i, DSP_OP_STORE)) return false;
    const dsp_op* pk = pick ? &ops[2] : nullptr;
    const dsp_op* am = amp ? &ops[pick ? 3 : 2] : nullptr;
    const dsp_op& first = pk ? *pk : *am;
    const dsp_op* ld = ops[0].dst == first.src ? &ops[0] : (ops[1].dst == first.src ? &ops[1] : nullptr);
    PulsesArgs& A = ch->only.pulses;
    if (!ld || !bind_rows(c, *ld, ROWS_F32_LOOP, ROWS_F64, A, why,
                          "the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"))
        return false;
    *why = "the list is loaded whole into slot ip[0], a list per row in the loop's type";
    const dsp_op* lt = ld == &ops[0] ? &ops[1] : &ops[0];
    if (first.ip[0] != lt->dst || lt->dst == first.src || lt->ip[0] != 0 || lt->ip[1] != 0 || io[lt->io].dtype != c.compute_dtype || io[lt->io].len != c.slot_len[lt->dst])
        return false;
    bind_raw(c, A.list, lt->io);
    A.list_stride = io[lt->io].row_stride;
    A.list_offset = io[lt->io].offset;
    *why = "multi_a_filter in the same program reads the same row at exactly the picker's idx_out";
    if (pk && am && (am->src != pk->src || am->ip[0] != pk->dst)) return false;
    *why = "idx_out and va_max_out are stored once each, whole, in the loop's type; the count once, into a DSP_U32 column";
    for (int i = first_store; i < first_store + n_stores; ++i) {
        const dsp_op& st = ops[i];
        const dsp_io_desc& o = io[st.io];
        void** out = pk && st.src == pk->dst ? &A.idx_out : (am && st.src == am->dst ? &A.amp_out : nullptr);
        if (!out || is_bound(c, *out) || o.dtype != c.compute_dtype || o.len != c.slot_len[st.src]) return false;
        bind(c, *out, st.io);
        (out == &A.idx_out ? A.idx_stride : A.amp_stride) = o.row_stride;
    }
    if ((am && !is_bound(c, A.amp_out)) || (!am && !is_bound(c, A.idx_out)) || (is_bound(c, A.idx_out) && ch->bound_io(A.idx_out) == ch->bound_io(A.amp_out))) return false;
    if (pk) {
        const dsp_op& sc = ops[n - 1];
        if (sc.ip[0] != pk->ip[1] || io[sc.io].dtype != DSP_U32) return false;
        bind(c, A.n_out, sc.io);
        A.n_stride = io[sc.io].row_stride;
        *why = "ratio_in is a constant or a per-event column of the loop's type";
        if (!bind_operand(c, *pk, 0, A.ratio, A.ratio_stride, A.ratio_const)) return false;
        A.width = dsp_pulses::clamped_width(op_const(c, *pk, 1), A.len);
    }
    A.m = c.slot_len[first.ip[0]];
    A.pick = pk ? 1 : 0;
    A.amp = am ? 1 : 0;
    return true;
}

// Is the program one of the decay-tail fitter's (dsp_tailfit.hip)?
//   LOAD s;  LOG_CHECK of s;  STORE of the logged row
//   LOAD s;  POLY_FIT of s;  STORE of the coefficients
//   LOAD s;  LOAD of the coefficients, a row of m per event;  POLY_DIFF | POLY_EXP_RMS of s and of them;  STORE_SCALAR, STORE_SCALAR
//   LOAD s;  [LOG_CHECK of s;]  POLY_FIT of the logged row (of s);  [STORE of the logged row;]  STORE of the coefficients
//   LOAD s;  [LOG_CHECK of s;]  POLY_FIT;  POLY_DIFF | POLY_EXP_RMS of s or of the logged row with the fitted coefficients;
//            [STORE of the logged row;]  [STORE of the coefficients;]  STORE_SCALAR, STORE_SCALAR
// each with or without  BL_SUBTRACT s <- s  (bl_subtract.py, a constant or a column of the loop's type) behind the LOAD of s: done as the rows
// are read.  Lengths and limits are lower_op's business (every program that holds one of the ops passes there first).  Why not, otherwise: `why`.
static bool match_tailfit_shape(const PlanCtx& c, const char** why) {
    ChainPlan* ch = c.ch;
    const dsp_op* ops = c.ops;
    const dsp_io_desc* io = c.io;
    const int n = c.n_ops;
    *why = "the program must be exactly LOAD, LOG_CHECK, STORE; or LOAD, POLY_FIT, STORE; or LOAD, LOAD of the coefficients, POLY_DIFF | POLY_EXP_RMS, STORE_SCALAR, "
           "STORE_SCALAR; or LOAD, [LOG_CHECK,] POLY_FIT, [POLY_DIFF | POLY_EXP_RMS,] [STORE of the logged row,] [STORE of the coefficients,] [STORE_SCALAR, "
           "STORE_SCALAR] (a BL_SUBTRACT of the rows, in place, may follow their LOAD)";
    auto is = [&](int i, int opcode) { return i >= 0 && i < n && ops[i].opcode == opcode; };
    if (n < 3 || !is(0, DSP_OP_LOAD)) return false;
    // ---- behind the first LOAD: at most one more LOAD (the coefficients) and one BL_SUBTRACT, in either order
    int at = 1;
    const dsp_op *ld2 = nullptr, *bs = nullptr;
    for (; at < n; ++at) {
        if (is(at, DSP_OP_LOAD) && !ld2) ld2 = &ops[at];
        else if (is(at, DSP_OP_BL_SUBTRACT) && !bs) bs = &ops[at];
        else break;
    }
    const dsp_op* lg = is(at, DSP_OP_LOG_CHECK) ? &ops[at++] : nullptr;
    const dsp_op* ft = is(at, DSP_OP_POLY_FIT) ? &ops[at++] : nullptr;
    const dsp_op* rs = is(at, DSP_OP_POLY_DIFF) || is(at, DSP_OP_POLY_EXP_RMS) ? &ops[at++] : nullptr;
    if ((!lg && !ft && !rs) || (lg && rs && !ft) || (ld2 != nullptr) != (rs && !ft)) return false;
    const int first_store = at, n_stores = n - first_store - (rs ? 2 : 0);
    if (n_stores < 0 || n_stores > (lg ? 1 : 0) + (ft ? 1 : 0) || c.n_slots != 1 + (ld2 ? 1 : 0) + (lg ? 1 : 0) + (ft ? 1 : 0)) return false;
    for (int i = first_store; i < first_store + n_stores; ++i)
        if (!is(i, DSP_OP_STORE)) return false;
    if (rs && (!is(n - 2, DSP_OP_STORE_SCALAR) || !is(n - 1, DSP_OP_STORE_SCALAR))) return false;
    // ---- the rows: the LOAD the first of the ops reads
    const dsp_op& first = lg ? *lg : (ft ? *ft : *rs);
    const dsp_op* ld = ops[0].dst == first.src ? &ops[0] : (ld2 && ld2->dst == first.src ? ld2 : nullptr);
    const dsp_op* lp = ld2 ? (ld == &ops[0] ? ld2 : &ops[0]) : nullptr;
    TailfitArgs& A = ch->only.tailfit;
    if (!ld || (!ld2 && ld != &ops[0]) || !bind_rows(c, *ld, ROWS_F32_LOOP, ROWS_F64, A, why,
                                                     "the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"))
        return false;
    if (bs) {
        *why = "the BL_SUBTRACT behind the LOAD works on the rows in place (bl_subtract, ip[0] = 0), its baseline a constant or a per-event column of the loop's type";
        if (bs->dst != ld->dst || bs->src != ld->dst || bs->ip[0] != 0 || !bind_operand(c, *bs, 0, A.sub, A.sub_stride, A.sub_const)) return false;
        A.sub_mode = 1;
    }
    *why = "poly_fit in the same program reads exactly the logged row; the residuals the row as loaded or the logged row, with exactly the fitted coefficients";
    if (lg && ft && ft->src != lg->dst) return false;
    if (ft && rs && (rs->ip[0] != ft->dst || (rs->src != ld->dst && !(lg && rs->src == lg->dst)))) return false;
    if (lp) {
        *why = "the coefficients are loaded whole into slot ip[0], a row of them per event in the loop's type";
        if (rs->ip[0] != lp->dst || lp->dst == rs->src || lp->ip[0] != 0 || lp->ip[1] != 0 || io[lp->io].dtype != c.compute_dtype || io[lp->io].len != c.slot_len[lp->dst])
            return false;
        bind_raw(c, A.pars, lp->io);
        A.pars_stride = io[lp->io].row_stride;
        A.pars_offset = io[lp->io].offset;
    }
    *why = "the logged row and the coefficients are stored once each, whole, in the loop's type; the two results of the residuals once each, in the loop's type";
    for (int i = first_store; i < first_store + n_stores; ++i) {
        const dsp_op& st = ops[i];
        const dsp_io_desc& o = io[st.io];
        void** out = lg && st.src == lg->dst ? &A.out : (ft && st.src == ft->dst ? &A.pars_out : nullptr);
        if (!out || is_bound(c, *out) || o.dtype != c.compute_dtype || o.len != c.slot_len[st.src]) return false;
        bind(c, *out, st.io);
        (out == &A.out ? A.out_stride : A.pars_out_stride) = o.row_stride;
    }
    if ((lg && !ft && !is_bound(c, A.out)) || (ft && !rs && !is_bound(c, A.pars_out)) || (is_bound(c, A.out) && ch->bound_io(A.out) == ch->bound_io(A.pars_out))) return false;
    if (rs) {
        const dsp_op &s0 = ops[n - 2], &s1 = ops[n - 1];
        const dsp_op* mean = s0.ip[0] == rs->dst ? &s0 : (s1.ip[0] == rs->dst ? &s1 : nullptr);
        const dsp_op* rms = s0.ip[0] == rs->dst + 1 ? &s0 : (s1.ip[0] == rs->dst + 1 ? &s1 : nullptr);
        if (!mean || !rms || mean == rms || mean->io == rms->io || io[mean->io].dtype != c.compute_dtype || io[rms->io].dtype != c.compute_dtype) return false;
        bind(c, A.mean_out, mean->io);
        bind(c, A.rms_out, rms->io);
        A.mean_stride = io[mean->io].row_stride;
        A.rms_stride = io[rms->io].row_stride;
        A.resid = rs->opcode == DSP_OP_POLY_EXP_RMS ? 2 : 1;
        A.resid_log = lg && rs->src == lg->dst ? 1 : 0;
    }
    if (ft) bind(c, A.inv, ft->io);
    A.m = ft ? c.slot_len[ft->dst] : (rs ? c.slot_len[rs->ip[0]] : 0);
    A.log = lg ? 1 : 0;
    A.fit = ft ? 1 : 0;
    vector_stores(c, A.out_vec, A.out, A.out_stride);
    return true;
}

// Is the program one of the waveform aligner's (dsp_align.hip)?
//   LOAD s;  INL_CORRECTION of s;  STORE of its n samples
//   LOAD s;  WF_CENTROID of s;  STORE_SCALAR of its register
//   LOAD s;  WF_ALIGNMENT of s into a slot of `size` samples;  STORE of them
//   LOAD s;  WF_CORRECTION of s;  STORE of its n samples
//   LOAD s;  WF_ALIGNMENT of s;  WF_CORRECTION of the aligned row;  [STORE of the aligned row;]  STORE of the corrected row
// Parameters, lengths and indices are lower_op's business (every program that holds one of the ops passes there first).  Why not, otherwise: `why`.
static bool match_align_shape(const PlanCtx& c, const char** why) {
    ChainPlan* ch = c.ch;
    const dsp_op* ops = c.ops;
    const dsp_io_desc* io = c.io;
    const int n = c.n_ops;
    *why = "the program must be exactly LOAD, INL_CORRECTION, STORE; or LOAD, WF_CENTROID, STORE_SCALAR; or LOAD, WF_ALIGNMENT, STORE; or LOAD, WF_CORRECTION, STORE; "
           "or LOAD, WF_ALIGNMENT, WF_CORRECTION, [STORE of the aligned row,] STORE";
    auto is = [&](int i, int opcode) { return i >= 0 && i < n && ops[i].opcode == opcode; };
    if (n < 3 || !is(0, DSP_OP_LOAD)) return false;
    const dsp_op &ld = ops[0], &op = ops[1];
    const dsp_op* cr = is(1, DSP_OP_WF_ALIGNMENT) && is(2, DSP_OP_WF_CORRECTION) ? &ops[2] : nullptr;
    const int first_store = cr ? 3 : 2, n_stores = n - first_store;
    if (op.src != ld.dst || (cr ? n_stores != 1 && n_stores != 2 : n_stores != 1) || c.n_slots != (is(1, DSP_OP_WF_CENTROID) ? 1 : (cr ? 3 : 2))) return false;
    for (int i = first_store; i < n; ++i)
        if (!is(i, is(1, DSP_OP_WF_CENTROID) ? DSP_OP_STORE_SCALAR : DSP_OP_STORE)) return false;
    AlignArgs& A = ch->only.align;
    constexpr unsigned INTS = 1u << DSP_I16 | 1u << DSP_U16 | 1u << DSP_I32 | 1u << DSP_U32;
    unsigned f32_rows = ROWS_F32_LOOP, f64_rows = ROWS_F64;
    const char* type_why = "the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows";
    switch (op.opcode) {
        case DSP_OP_INL_CORRECTION:
            A.mode = DSP_ALIGN_INL;
            f32_rows = f64_rows = INTS;
            type_why = "inl_correction reads DSP_I16, DSP_U16, DSP_I32 or DSP_U32 rows: an ADC code is an integer";
            break;
        case DSP_OP_WF_CENTROID: A.mode = DSP_ALIGN_CENTROID; break;
        case DSP_OP_WF_ALIGNMENT:
            A.mode = DSP_ALIGN_WINDOW;
            f64_rows |= INTS;  // (the float32 loop: int16 and uint16, which a float32 holds exactly -- int32 rows select the float64 loop, as everywhere)
            type_why = "wf_alignment takes the loop's float rows, DSP_I16 or DSP_U16 rows in either loop, DSP_I32 or DSP_U32 rows in the float64 loop";
            break;
        case DSP_OP_WF_CORRECTION: A.mode = DSP_ALIGN_CORRECT; break;
        default: return false;
    }
    if (!bind_rows(c, ld, f32_rows, f64_rows, A, why, type_why)) return false;
    A.f64 = c.f64 ? 1 : 0;
    if (A.mode == DSP_ALIGN_CENTROID) {
        const dsp_op& sc = ops[2];
        *why = "the centroid is stored once, into a column of the loop's type";
        if (sc.ip[0] != op.dst || io[sc.io].dtype != c.compute_dtype) return false;
        bind(c, A.scalar_out, sc.io);
        A.scalar_stride = io[sc.io].row_stride;
        A.shift = op_const(c, op, 0);
        return true;
    }
    if (A.mode == DSP_ALIGN_WINDOW) {
        *why = "centroid is a constant or a per-event column of the loop's type";
        if (!bind_operand(c, op, 0, A.centroid, A.centroid_stride, A.centroid_const)) return false;
        A.shift = op_const(c, op, 1);
        A.size = c.slot_len[op.dst];
    }
    const dsp_op& tb = cr ? *cr : op;  // the op with a table
    if (tb.opcode != DSP_OP_WF_ALIGNMENT) {
        bind(c, A.table, tb.io);
        A.table_len = io[tb.io].len;
        A.start = tb.ip[0];
        A.stop = tb.ip[1];
    }
    *why = "wf_correction in the same program reads exactly the aligned row";
    if (cr && (cr->src != op.dst || cr->dst == op.dst)) return false;
    A.correct = cr ? 1 : 0;
    *why = "each output row is stored once, whole, in the loop's type";
    for (int i = first_store; i < n; ++i) {
        const dsp_op& st = ops[i];
        const dsp_io_desc& o = io[st.io];
        void** out = cr && st.src == cr->dst ? &A.out2 : (st.src == op.dst ? &A.out : nullptr);
        if (!out || is_bound(c, *out) || o.dtype != c.compute_dtype || o.len != c.slot_len[st.src]) return false;
        bind(c, *out, st.io);
        (out == &A.out ? A.out_stride : A.out2_stride) = o.row_stride;
    }
    if (cr ? !is_bound(c, A.out2) || ch->bound_io(A.out2) == ch->bound_io(A.out) : !is_bound(c, A.out)) return false;
    if (A.mode != DSP_ALIGN_WINDOW) vector_stores(c, A.out_vec, A.out, A.out_stride);  // (the outputs the kernel streams: inl_correction's, wf_correction's)
    return true;
}

// what dsp_chain_geometry reports of a launch: LDS per wavefront, wavefronts per block, blocks for n_wf rows
struct Geometry {
    int lds, wpb;
    int64_t blocks;
};
// The routes that are no optimisation: ops the interpreter has no case for, a row per route and everything HIP-free about the route in it.
// A program that holds one of `opcodes` has the shape `match` accepts, or is refused with `refusal` and the matcher's reason.  (A program
// never matches two: every shape is exact.)  `lds`: the dynamic LDS of a launch where the kernel's limit may have to be raised for it (null:
// the route has no limit to raise); `geometry`: the launch as dsp_chain_geometry reports it.  dsp_host.cpp's kernel_only_launches holds
// the HIP side, a row per route again.
struct KernelOnlyRoute {
    dsp_route route;
    int opcodes[4];  // (0: none)
    bool (*match)(const PlanCtx& c, const char** why);
    const char* refusal;
    int (*lds)(const ChainPlan& p);
    Geometry (*geometry)(const ChainPlan& p, int64_t n_wf);
};
static int loop_esz(const ChainPlan& p) { return p.f64 ? 8 : 4; }
// a wavefront per row, four rows to a workgroup, `lds` bytes each ...
static Geometry wave_per_row(int lds, int64_t n_wf) { return {lds, 4, (n_wf + 3) / 4}; }
// ... or, a row too long for that, a workgroup of four wavefronts per row
static Geometry row_in_lds(int row_bytes, bool wide, int64_t n_wf) { return wide ? Geometry{row_bytes / 4, 4, n_wf} : wave_per_row(row_bytes, n_wf); }
static Geometry rows_from_memory(const ChainPlan&, int64_t n_wf) { return wave_per_row(0, n_wf); }
static constexpr KernelOnlyRoute kernel_only_routes[] = {
    {DSP_ROUTE_EXTREMA, {DSP_OP_MULTI_EXTREMA, DSP_OP_MULTI_EXTREMA}, match_extrema_shape,
     "DSP_OP_MULTI_EXTREMA (get_multi_local_extrema) runs on dsp_extrema_kernel only", nullptr, rows_from_memory},
    {DSP_ROUTE_HIST, {DSP_OP_HISTOGRAM, DSP_OP_HISTOGRAM_STATS}, match_hist_shape,
     "DSP_OP_HISTOGRAM / DSP_OP_HISTOGRAM_STATS (histogram, histogram_stats) run on dsp_hist_kernel only", nullptr,
     [](const ChainPlan& p, int64_t n_wf) { return wave_per_row(dsp_hist::lds_bytes(p.only.hist.m) / 4, n_wf); }},
    {DSP_ROUTE_THRESH, {DSP_OP_MULTI_TIME_POINT_THRESH, DSP_OP_TIME_OVER_THRESHOLD}, match_thresh_shape,
     "DSP_OP_MULTI_TIME_POINT_THRESH / DSP_OP_TIME_OVER_THRESHOLD (multi_time_point_thresh, time_over_threshold) run on dsp_thresh_kernel only",
     nullptr, rows_from_memory},
    {DSP_ROUTE_SPECTRUM, {DSP_OP_PSD, DSP_OP_FFT}, match_spectrum_shape, "DSP_OP_PSD / DSP_OP_FFT (psd, fft) run on dsp_spectrum_kernel only",
     [](const ChainPlan& p) { return dsp_spectrum::lds_bytes(p.only.spec.len, loop_esz(p)); },
     [](const ChainPlan& p, int64_t n_wf) {
         const int n = p.only.spec.len, es = loop_esz(p);
         return row_in_lds(dsp_spectrum::row_bytes(n, es), dsp_spectrum::wide(n, es), n_wf);
     }},
    {DSP_ROUTE_SORT, {DSP_OP_SORT, DSP_OP_SORT}, match_sort_shape, "DSP_OP_SORT (sort) runs on dsp_sort_kernel only",
     [](const ChainPlan& p) { return dsp_sort::lds_bytes(p.only.sort.len, loop_esz(p)); },
     [](const ChainPlan& p, int64_t n_wf) {
         const int n = p.only.sort.len;
         return row_in_lds(dsp_sort::padded(n) * loop_esz(p), dsp_sort::wide(n), n_wf);
     }},
    {DSP_ROUTE_INTERP, {DSP_OP_INTERP_UPSAMPLE, DSP_OP_INTERP_UPSAMPLE}, match_interp_shape,
     "DSP_OP_INTERP_UPSAMPLE (interpolating_upsampler) runs on dsp_interp_kernel only",
     [](const ChainPlan& p) { return dsp_interp::lds_bytes(p.only.interp.mode, p.only.interp.len, loop_esz(p)); },
     [](const ChainPlan& p, int64_t n_wf) {
         const int n = p.only.interp.len, mode = p.only.interp.mode, es = loop_esz(p);
         return row_in_lds(dsp_interp::row_bytes(mode, n, es), dsp_interp::wide(mode, n, es), n_wf);
     }},
    {DSP_ROUTE_DENSE, {DSP_OP_NORMALISE, DSP_OP_DENSE}, match_dense_shape,
     "DSP_OP_NORMALISE / DSP_OP_DENSE (normalisation_layer, dense_layer_*, classification_layer_*) run on dsp_dense_kernel only",
     [](const ChainPlan& p) { return dsp_dense::lds_bytes(p.only.dense.m, loop_esz(p)); },
     [](const ChainPlan& p, int64_t n_wf) {  // a tile of 64 rows per workgroup; the normalisation alone: a wavefront per row
         const int m = p.only.dense.m;
         return m > 0 ? Geometry{dsp_dense::lds_bytes(m, loop_esz(p)) / 4, 4, dsp_dense::tiles(n_wf)} : wave_per_row(0, n_wf);
     }},
    {DSP_ROUTE_REFLECT, {DSP_OP_REFLECTED_CONVOLVE, DSP_OP_REFLECTED_CONVOLVE}, match_reflect_shape,
     "DSP_OP_REFLECTED_CONVOLVE (reflected_convolve_wf) runs on dsp_reflect_kernel only",
     [](const ChainPlan& p) { return dsp_reflect::lds_bytes(p.only.reflect.len, p.only.reflect.n_taps, loop_esz(p)); },
     [](const ChainPlan& p, int64_t n_wf) {
         const int n = p.only.reflect.len, m = p.only.reflect.n_taps, es = loop_esz(p);
         return row_in_lds(dsp_reflect::row_bytes(n, m, es), dsp_reflect::wide(n, m, es), n_wf);
     }},
    {DSP_ROUTE_PILEUP, {DSP_OP_RC_CR2, DSP_OP_BI_LEVEL_ZERO_CROSSING}, match_pileup_shape,
     "DSP_OP_RC_CR2 / DSP_OP_BI_LEVEL_ZERO_CROSSING (rc_cr2, bi_level_zero_crossing_time_points) run on dsp_pileup_kernel only", nullptr,
     [](const ChainPlan& p, int64_t n_wf) {  // a tile of 64 rows per wavefront, one wavefront a workgroup
         return Geometry{dsp_pileup::lds_bytes(loop_esz(p)), 1, dsp_pileup::tiles(n_wf)};
     }},
    {DSP_ROUTE_PULSES, {DSP_OP_PEAK_SNR_THRESHOLD, DSP_OP_MULTI_A_FILTER}, match_pulses_shape,
     "DSP_OP_PEAK_SNR_THRESHOLD / DSP_OP_MULTI_A_FILTER (peak_snr_threshold, multi_a_filter) run on dsp_pulses_kernel only", nullptr, rows_from_memory},
    {DSP_ROUTE_TAILFIT, {DSP_OP_LOG_CHECK, DSP_OP_POLY_FIT, DSP_OP_POLY_DIFF, DSP_OP_POLY_EXP_RMS}, match_tailfit_shape,
     "DSP_OP_LOG_CHECK / DSP_OP_POLY_FIT / DSP_OP_POLY_DIFF / DSP_OP_POLY_EXP_RMS (log_check, poly_fit, poly_diff, poly_exp_rms) run on dsp_tailfit_kernel only",
     nullptr, [](const ChainPlan& p, int64_t n_wf) {  // the pile-up kernel's tile, and the table of powers beside it
         return Geometry{dsp_tailfit::lds_bytes(loop_esz(p)), 1, dsp_tailfit::tiles(n_wf)};
     }},
    {DSP_ROUTE_ALIGN, {DSP_OP_INL_CORRECTION, DSP_OP_WF_CENTROID, DSP_OP_WF_ALIGNMENT, DSP_OP_WF_CORRECTION}, match_align_shape,
     "DSP_OP_INL_CORRECTION / DSP_OP_WF_CENTROID / DSP_OP_WF_ALIGNMENT / DSP_OP_WF_CORRECTION (inl_correction, get_wf_centroid, wf_alignment, wf_correction) run on dsp_align_kernel only",
     nullptr, rows_from_memory},
    {DSP_ROUTE_SVM, {DSP_OP_SVM_PREDICT, DSP_OP_SVM_PREDICT}, match_svm_shape, "DSP_OP_SVM_PREDICT (svm_predict) runs on dsp_svm_kernel only",
     [](const ChainPlan& p) { return dsp_svm::lds_bytes(p.only.svm.len, p.only.svm.n_pairs); },
     [](const ChainPlan& p, int64_t n_wf) {  // the dense kernel's tile of 64 rows per workgroup
         return Geometry{dsp_svm::lds_bytes(p.only.svm.len, p.only.svm.n_pairs) / 4, 4, dsp_svm::tiles(n_wf)};
     }},
};
constexpr bool kernel_only_routes_in_order() {
    int n = 0;
    for (const KernelOnlyRoute& r : kernel_only_routes)
        if (r.route != n++) return false;
    return n == DSP_KERNEL_ONLY_ROUTES;
}
static_assert(kernel_only_routes_in_order(), "a row per kernel-only route, at the route's own index");

// Does the program have the shape of the current-branch kernel (dsp_current.hip)?
//   LOAD s0;  WINDOWER s1 <- s0 (start: constant or float32 column);  AVG_CURRENT s2 <- s1;  UPSAMPLER s3 <- s2;
//   MOVING_WINDOW_MULTI d <- s3 (3 windows, alternating);  MIN_MAX of d;  STORE_SCALARs of its four registers
static bool match_current_shape(const PlanCtx& c) {
    ChainPlan* ch = c.ch;
    const dsp_op* ops = c.ops;
    const dsp_io_desc* io = c.io;
    const int32_t* slot_len = c.slot_len;
    const int n_ops = c.n_ops;
    if (c.f64 || n_ops < 7) return false;
    const dsp_op &ld = ops[0], &wi = ops[1], &ac = ops[2], &up = ops[3], &mw = ops[4], &mm = ops[5];
    if (ld.opcode != DSP_OP_LOAD || wi.opcode != DSP_OP_WINDOWER || ac.opcode != DSP_OP_AVG_CURRENT || up.opcode != DSP_OP_UPSAMPLER ||
        mw.opcode != DSP_OP_MOVING_WINDOW_MULTI || mm.opcode != DSP_OP_MIN_MAX)
        return false;
    if (wi.src != ld.dst || ac.src != wi.dst || up.src != ac.dst || mw.src != up.dst || mm.src != mw.dst) return false;
    const dsp_io_desc& w = io[ld.io];
    if (w.dtype != DSP_F32 || ld.ip[0] != 0 || ld.ip[1] != 0 || (w.row_stride % 4) != 0 || (w.offset % 4) != 0 || (w.len % 4) != 0) return false;
    CurrentArgs& A = ch->cur;
    memset(&A, 0, sizeof A);
    A.wf_stride = w.row_stride;
    A.wf_offset = w.offset;
    A.n_in = w.len;
    A.scan_rows = (ld.ip[2] & 1) ? 0 : 1;
    if (wi.sp[0].kind == DSP_ARG_INPUT && io[wi.sp[0].index].dtype == DSP_F32) {
        ch->cio_t0 = wi.sp[0].index;
        A.t0_stride = io[ch->cio_t0].row_stride;
    } else if (wi.sp[0].kind == DSP_ARG_CONST) {
        A.t0_const = (float)wi.sp[0].value;
    } else {
        return false;
    }
    A.win_len = slot_len[wi.dst];
    if (A.win_len < 2 || A.win_len >= A.n_in) return false;
    // avg_current: an integer-valued length inside the window
    if (ac.sp[0].kind != DSP_ARG_CONST) return false;
    const float acl = (float)ac.sp[0].value;
    if (!(acl >= 1.0f) || std::floor(acl) != acl || acl >= (float)A.win_len) return false;
    A.ac_lag = (int)acl;
    A.ac_length = acl;
    A.n_c = A.win_len - A.ac_lag;
    if (slot_len[ac.dst] != A.n_c) return false;
    // upsampler: a factor in {1, 2, 4, 8, 16}, every output sample reached by an input sample
    if (up.sp[0].kind != DSP_ARG_CONST) return false;
    const float upf = (float)up.sp[0].value;
    int shift = -1;
    for (int k = 0; k <= 4; ++k)
        if (upf == (float)(1 << k)) shift = k;
    if (shift < 0) {
        note(ch, "the current branch with an upsampling factor of %g: the lane-per-waveform kernel takes 1, 2, 4, 8 or 16", (double)upf);
        return false;
    }
    A.up_shift = shift;
    A.up_half = (1 << shift) / 2;
    A.n_up = slot_len[up.dst];
    if (A.n_up < 32 || A.n_up % 16 != 0 || ((A.n_up - 1 + A.up_half) >> shift) >= A.n_c) {
        if (A.n_up % 16 != 0) note(ch, "the current branch with %d upsampled samples: the lane-per-waveform kernel takes a multiple of 16", A.n_up);
        return false;
    }
    // moving_window_multi: three alternating windows whose length is a multiple of 16 samples
    if (mw.sp[0].kind != DSP_ARG_CONST || mw.ip[0] != 0 || mw.ip[1] != 3 || slot_len[mw.dst] != A.n_up) {
        if (mw.sp[0].kind == DSP_ARG_CONST && (mw.ip[0] != 0 || mw.ip[1] != 3))
            note(ch, "the current branch with %d moving windows of type %d: the lane-per-waveform kernel takes three alternating ones", mw.ip[1], mw.ip[0]);
        return false;
    }
    const float mal = (float)mw.sp[0].value;
    if (!(mal >= 16.0f) || std::floor(mal) != mal || mal > 112.0f || ((int)mal % 16) != 0 || (int)mal >= A.n_up) {
        note(ch, "the current branch with moving windows of %g samples: the lane-per-waveform kernel takes multiples of 16 up to 112", (double)mal);
        return false;
    }
    A.ma_len = (int)mal;
    A.ma_length = mal;
    for (int i = 6; i < n_ops; ++i) {
        const dsp_op& o = ops[i];
        if (o.opcode != DSP_OP_STORE_SCALAR || io[o.io].dtype != DSP_F32) return false;
        const int k = o.ip[0] - mm.dst;
        if (k < 0 || k > 3 || ch->cio_out[k] >= 0) return false;
        ch->cio_out[k] = o.io;
        A.out_stride[k] = io[o.io].row_stride;
    }
    A.scratch_per_wave = (int64_t)(A.n_c + 2 * (A.n_up / 16)) * 64;
    ch->cio_wf = ld.io;
    ch->cur_lds_bytes = dsp_current::lds_bytes(A.ma_len);
    return true;
}

static bool match_fir_shape(const PlanCtx& c) {
    ChainPlan* ch = c.ch;
    const dsp_op* ops = c.ops;
    const dsp_io_desc* io = c.io;
    const int32_t* slot_len = c.slot_len;
    const int n_ops = c.n_ops, n_slots = c.n_slots;
    if (c.f64 || n_ops < 3 || n_slots != 1 || ops[0].opcode != DSP_OP_LOAD) return false;
    const dsp_op& ld = ops[0];
    const int s = ld.dst, wdt = io[ld.io].dtype, n = slot_len[s];
    if (wdt != DSP_F32 && wdt != DSP_I16 && wdt != DSP_U16) return false;
    const int es = wdt == DSP_F32 ? 4 : 2, align = wdt == DSP_F32 ? 16 : 8;  // 4 samples per staging load
    if ((io[ld.io].row_stride * es) % align != 0 || (io[ld.io].offset * es) % align != 0) return false;
    FirArgs& A = ch->fir;
    memset(&A, 0, sizeof A);
    int i = 1;
    if (ops[i].opcode == DSP_OP_BL_SUBTRACT) {
        const dsp_op& bs = ops[i++];
        if (bs.dst != s || bs.src != s) return false;
        if (bs.sp[0].kind == DSP_ARG_INPUT && io[bs.sp[0].index].dtype == DSP_F32) {
            ch->fio_bl = bs.sp[0].index;
            A.bl_stride = io[ch->fio_bl].row_stride;
        } else if (bs.sp[0].kind == DSP_ARG_CONST) {
            A.bl_const = (float)bs.sp[0].value;
        } else {
            return false;
        }
        A.sub_mode = 1;
    }
    int regs[DSP_FIR_MAXK], nk = 0, max_m = 0;
    for (; i < n_ops && ops[i].opcode == DSP_OP_CONVOLVE_AMAX; ++i) {
        const dsp_op& o = ops[i];
        if (nk == DSP_FIR_MAXK || o.src != s || o.ip[0] != 'v' || o.ip[1] != 0 || io[o.io].dtype != DSP_F32) return false;
        const int m = o.ip[3] > 0 ? o.ip[3] : io[o.io].len, p = n - m + 1;
        if (m < 64 || p < 1 || p > 320 || o.ip[2] != p) {  // (a short kernel is the VM's business)
            if (m < 64) note(ch, "a %d-tap 'valid' convolution and its maximum: the matrix-core FIR takes kernels of 64 taps and more", m);
            else if (p > 320) note(ch, "'valid' convolution with %d outputs and their maximum: the matrix-core FIR with a maximum takes up to 320", p);
            return false;
        }
        ch->fio_taps[nk] = o.io;
        A.m[nk] = m;
        A.p[nk] = p;
        regs[nk] = o.dst;
        if (m > max_m) max_m = m;
        ++nk;
    }
    if (nk == 0) return false;
    for (; i < n_ops; ++i) {
        const dsp_op& o = ops[i];
        if (o.opcode != DSP_OP_STORE_SCALAR || io[o.io].dtype != DSP_F32) return false;
        int k = 0;
        while (k < nk && (regs[k] != o.ip[0] || ch->fio_out[k] >= 0)) ++k;
        if (k == nk) return false;
        ch->fio_out[k] = o.io;
        A.out_stride[k] = io[o.io].row_stride;
    }
    for (int k = 0; k < nk; ++k)
        if (ch->fio_out[k] < 0) return false;
    int kend = n < 319 + max_m ? n : 319 + max_m;
    kend = ((kend + 31) / 32) * 32;
    if (io[ld.io].offset + kend > io[ld.io].row_stride) return false;  // the staging loads run to the end of the last 32-sample stage
    A.wf_stride = io[ld.io].row_stride;
    A.wf_offset = io[ld.io].offset;
    A.n = n;
    A.in_kind = wdt == DSP_F32 ? 0 : (wdt == DSP_I16 ? 1 : 2);
    A.n_kernels = nk;
    A.kend = kend;
    A.scan_before = ld.ip[0];
    A.scan_after = ld.ip[1];
    ch->fio_wf = ld.io;
    ch->fir_lds_bytes = dsp_fir_mfma::lds_bytes(kend);
    return ch->fir_lds_bytes <= 80 * 1024;
}

// The matrix-core FIR with its output kept (dsp_fir_store_kernel):  LOAD s; [BL_SUBTRACT s <- s]; CONVOLVE d <- s (any mode, >= 64 finite taps);
// STORE d.  What whole recipes run ahead of their program for the filters other processors read (the t0 filter).
static bool match_fir_store_shape(const PlanCtx& c) {
    ChainPlan* ch = c.ch;
    const dsp_op* ops = c.ops;
    const dsp_io_desc* io = c.io;
    const int32_t* slot_len = c.slot_len;
    const int n_ops = c.n_ops, n_slots = c.n_slots;
    if (c.f64 || n_ops < 3 || n_ops > 4 || n_slots != 2 || ops[0].opcode != DSP_OP_LOAD) return false;
    const dsp_op& ld = ops[0];
    const int s = ld.dst, wdt = io[ld.io].dtype, n = slot_len[s];
    if (wdt != DSP_F32 && wdt != DSP_I16 && wdt != DSP_U16) return false;
    const int es = wdt == DSP_F32 ? 4 : 2, align = wdt == DSP_F32 ? 16 : 8;
    if ((io[ld.io].row_stride * es) % align != 0 || (io[ld.io].offset * es) % align != 0) return false;
    FirArgs& A = ch->fir;
    memset(&A, 0, sizeof A);
    ch->fio_bl = -1;
    int i = 1;
    if (ops[i].opcode == DSP_OP_BL_SUBTRACT) {
        const dsp_op& bs = ops[i++];
        if (bs.dst != s || bs.src != s || bs.ip[0] != 0) return false;
        if (bs.sp[0].kind == DSP_ARG_INPUT && io[bs.sp[0].index].dtype == DSP_F32) {
            ch->fio_bl = bs.sp[0].index;
            A.bl_stride = io[ch->fio_bl].row_stride;
        } else if (bs.sp[0].kind == DSP_ARG_CONST) {
            A.bl_const = (float)bs.sp[0].value;
        } else {
            return false;
        }
        A.sub_mode = 1;
    }
    if (i + 2 != n_ops || ops[i].opcode != DSP_OP_CONVOLVE || ops[i + 1].opcode != DSP_OP_STORE) return false;
    const dsp_op& o = ops[i];
    const dsp_op& st = ops[i + 1];
    if (o.src != s || o.dst == s || (o.ip[1] & 3) != 0 || io[o.io].dtype != DSP_F32 || st.src != o.dst || io[st.io].dtype != DSP_F32) return false;
    const int m = o.ip[3] > 0 ? o.ip[3] : io[o.io].len;
    if (m < 64 || m > n) {
        if (m < 64) note(ch, "a %d-tap convolution: the matrix-core FIR takes kernels of 64 taps and more", m);
        return false;
    }
    const int mode = o.ip[0];
    const int P = mode == 'v' ? n - m + 1 : (mode == 's' ? n : (mode == 'f' ? n + m - 1 : -1));
    if (P < 1 || slot_len[o.dst] != P || io[st.io].len != P) return false;
    A.store = 1;
    A.dshift = mode == 'v' ? 0 : (mode == 's' ? m / 2 : m - 1);
    A.m[0] = m;
    A.p[0] = P;
    A.n_kernels = 1;
    A.out_stride[0] = io[st.io].row_stride;
    A.wf_stride = io[ld.io].row_stride;
    A.wf_offset = io[ld.io].offset;
    A.n = n;
    A.in_kind = wdt == DSP_F32 ? 0 : (wdt == DSP_I16 ? 1 : 2);
    A.kend = ((320 + m - 1 + 3 + 31) / 32) * 32;  // the longest window of a 320-column tile (dsp_fir_mfma.hip)
    A.scan_before = ld.ip[0];
    A.scan_after = ld.ip[1];
    ch->fio_wf = ld.io;
    ch->fio_taps[0] = o.io;
    ch->fio_out[0] = st.io;
    ch->fir_lds_bytes = dsp_fir_mfma::store_lds_bytes(A.kend);
    return ch->fir_lds_bytes <= 80 * 1024;
}

// The run-length FIR (dsp_fir_runs.hip):  LOAD s (float32 rows);  CONVOLVE d <- s with ip[2] = 1 (the caller found the kernel piecewise constant:
// at most DSP_FIR_RUNS_MAX runs) and at most DSP_FIR_RUNS_MAX_TAPS finite taps, any mode;  [STORE d];  [the reductions of match_reduce_ops on d].
// At least one of the two: a filtered waveform nobody keeps and nobody reads is no program.
static bool match_fir_runs_shape(const PlanCtx& c) {
    ChainPlan* ch = c.ch;
    const dsp_op* ops = c.ops;
    const dsp_io_desc* io = c.io;
    const int32_t* slot_len = c.slot_len;
    const int n_ops = c.n_ops, n_slots = c.n_slots;
    if (c.f64 || n_ops < 3 || n_slots != 2 || ops[0].opcode != DSP_OP_LOAD || ops[1].opcode != DSP_OP_CONVOLVE) return false;
    const dsp_op &ld = ops[0], &o = ops[1];
    const dsp_io_desc& w = io[ld.io];
    const int s = ld.dst, n = slot_len[s];
    if (o.ip[2] != 1 || (o.ip[1] & 3) != 0 || o.src != s || o.dst == s || io[o.io].dtype != DSP_F32) return false;
    if (w.dtype != DSP_F32 || ld.ip[0] != 0 || ld.ip[1] != 0 || w.len != n || n % 8 != 0 || n < 8 || w.row_stride % 4 != 0 || w.offset % 4 != 0) {
        note(ch, "a piecewise-constant kernel on rows that are not float32, 16-byte aligned and a multiple of 8 samples long: the run-length FIR kernel takes those");
        return false;
    }
    const int m = o.ip[3] > 0 ? o.ip[3] : io[o.io].len;
    if (m < 1 || m > n || m > DSP_FIR_RUNS_MAX_TAPS) return false;
    const int mode = o.ip[0];
    const int P = mode == 'v' ? n - m + 1 : (mode == 's' ? n : (mode == 'f' ? n + m - 1 : -1));
    if (P < 1 || slot_len[o.dst] != P) return false;
    FirRunsArgs& A = ch->runs;
    memset(&A, 0, sizeof A);
    // the STORE of the filtered waveform, wherever it stands behind the CONVOLVE; everything else must be the reductions and their stores
    ch->uio_out = -1;
    std::vector<dsp_op> rest;
    for (int i = 2; i < n_ops; ++i) {
        if (ops[i].opcode == DSP_OP_STORE) {
            const dsp_op& st = ops[i];
            if (A.keep || st.src != o.dst || io[st.io].dtype != DSP_F32 || io[st.io].len != P) return false;
            ch->uio_out = st.io;
            A.keep = 1;
            A.out_stride = io[st.io].row_stride;
        } else {
            rest.push_back(ops[i]);
        }
    }
    for (int k = 0; k < 5; ++k) ch->dio_out[k] = -1;
    for (int k = 0; k < DSP_REDUCE_PICKS; ++k) ch->dio_pick[k] = -1;
    for (int k = 0; k < DSP_REDUCE_WALKS; ++k) ch->dio_walk[k] = ch->dio_walk_thr[k] = ch->dio_walk_ts[k] = -1;
    if (!rest.empty()) {
        if (!match_reduce_ops(ch, rest.data(), 0, (int)rest.size(), o.dst, P, io, A.red)) return false;
        A.red.need_stream = 1;
        A.has_red = 1;
    } else if (!A.keep) {
        return false;
    }
    A.wf_stride = w.row_stride;
    A.wf_offset = w.offset;
    A.n = n;
    A.m = m;
    A.p = P;
    A.start = mode == 'v' ? m - 1 : (mode == 's' ? (m - 1) / 2 : 0);
    if (!A.keep) A.out_stride = (P + 63) & ~63;  // the pitch of the wavefronts' scratch rows
    ch->uio_wf = ld.io;
    ch->uio_taps = o.io;
    return true;
}

// Does the program have the shape of the lane-per-waveform kernel?  Fills ch->rows / ch->rio_* and returns true if so.
//   LOAD s;  [BL_SUBTRACT s <- s];  POLE_ZERO | DOUBLE_POLE_ZERO s <- s;  then in any order: one TRAP_REDUCE of s, at most one DWT_HAAR of s
//   into a slot that is stored, STORE_SCALARs of the reduction's registers.
static bool match_rows_shape(const PlanCtx& c) {
    ChainPlan* ch = c.ch;
    const dsp_op* ops = c.ops;
    const dsp_io_desc* io = c.io;
    const int32_t* slot_len = c.slot_len;
    const int n_ops = c.n_ops, n_slots = c.n_slots;
    const DevProgram& P = ch->host;
    if (c.f64 || n_ops < 3 || n_slots < 1 || n_slots > 2) return false;
    int i = 0;
    if (ops[i].opcode != DSP_OP_LOAD) return false;
    const dsp_op& ld = ops[i++];
    const int s = ld.dst;
    const int wdt = io[ld.io].dtype, len = slot_len[s];
    if (ld.ip[0] != 0 || ld.ip[1] != 0) return false;
    const bool row_layout = (wdt == DSP_F32 || wdt == DSP_I16 || wdt == DSP_U16) && P.io[ld.io].vec_ok && len % 8 == 0 && len >= 16;
    auto f32_or_const = [&](const dsp_scalar_arg& a) { return a.kind == DSP_ARG_CONST || (a.kind == DSP_ARG_INPUT && io[a.index].dtype == DSP_F32); };
    const dsp_op* bs = nullptr;
    if (ops[i].opcode == DSP_OP_BL_SUBTRACT) {
        bs = &ops[i++];
        if (bs->dst != s || bs->src != s || !f32_or_const(bs->sp[0])) return false;
    }
    if (i >= n_ops) return false;
    // (no pole-zero step at all: the rows are a waveform another program already corrected -- what whole recipes stage in HBM)
    const bool has_pz = ops[i].opcode == DSP_OP_POLE_ZERO || ops[i].opcode == DSP_OP_DOUBLE_POLE_ZERO;
    const dsp_op& pz = ops[has_pz ? i : 0];
    const DevOp& dpz = P.ops[c.dev_index[has_pz ? i : 0]];
    if (has_pz) {
        ++i;
        if (pz.dst != s || pz.src != s) return false;
        for (int k = 0; k < (pz.opcode == DSP_OP_POLE_ZERO ? 1 : 3); ++k)
            if (pz.sp[k].kind != DSP_ARG_CONST) {  // (per-event time constants: the VM's ops form the coefficients per row)
                note(ch, "a pole-zero time constant per event: the lane-per-waveform rows kernel takes constants");
                return false;
            }
    }
    const dsp_op *tr = nullptr, *dw = nullptr, *st_wf = nullptr;
    int tr_at = -1;
    std::vector<const dsp_op*> st_sc;
    for (; i < n_ops; ++i) {
        const dsp_op& o = ops[i];
        if (o.opcode == DSP_OP_TRAP_REDUCE && !tr && o.src == s) {
            tr = &o;
            tr_at = i;
        } else if (o.opcode == DSP_OP_DWT_HAAR && !dw && o.src == s && o.dst != s) {
            dw = &o;
        } else if (o.opcode == DSP_OP_STORE_SCALAR) {
            st_sc.push_back(&o);
        } else if (o.opcode == DSP_OP_STORE && !st_wf) {
            st_wf = &o;
        } else {
            return false;
        }
    }
    if (!tr || (dw != nullptr) != (st_wf != nullptr)) return false;
    if (tr->ip[3] >> 8) return false;  // (a pick-off or the amax-only form of the reduction: the VM's)
    if (dw && (st_wf->src != dw->dst || io[st_wf->io].dtype != DSP_F32)) return false;
    if (!row_layout) {
        note(ch, "rows of %d samples: the lane-per-waveform rows kernel takes float32 / int16 / uint16 rows of a multiple of 8 samples (16 and more) that start on 16-byte boundaries", len);
        return false;
    }
    const DevOp& dtr = P.ops[c.dev_index[tr_at]];
    RowsArgs& A = ch->rows;
    memset(&A, 0, sizeof A);
    A.wf_stride = io[ld.io].row_stride;
    A.wf_offset = io[ld.io].offset;
    A.len = len;
    A.in_kind = wdt == DSP_F32 ? 0 : (wdt == DSP_I16 ? 1 : 2);
    ch->rio_wf = ld.io;
    if (bs) {
        A.sub_mode = 1;
        if (bs->sp[0].kind == DSP_ARG_INPUT) {
            ch->rio_bl = bs->sp[0].index;
            A.bl_stride = io[ch->rio_bl].row_stride;
        } else {
            A.bl_const = (float)bs->sp[0].value;
        }
    }
    A.pz_kind = !has_pz ? 0 : (pz.opcode == DSP_OP_POLE_ZERO ? 1 : 2);
    A.pz_param_nan = has_pz ? dpz.ic[0] : 0;
    if (A.pz_kind == 0) {
        if (dw) return false;  // (the Haar transform of the kernel is the one of the pole-zero output)
    } else if (A.pz_kind == 1) {
        A.pz_c = dpz.fc[0];
    } else {
        A.n1 = dpz.fc[0];
        A.n2 = dpz.fc[1];
        A.d1 = dpz.fc[2];
        A.d2 = dpz.fc[3];
    }
    // trapezoid: every lag at least one block of the kernel (8 samples), the history ring within half a CU's LDS
    A.trap_kind = tr->ip[3] == DSP_OP_TRAP_FILTER ? 0 : (tr->ip[3] == DSP_OP_TRAP_NORM ? 1 : 2);
    int maxlag = 0;
    for (int k = 0; k < 3; ++k) {
        A.lag[k] = dtr.ic[k];
        if (A.lag[k] < dsp_rows::RB) {
            note(ch, "a trapezoid with a rise or flat top of %d samples: the lane-per-waveform rows kernel takes 8 and more", A.lag[k]);
            return false;
        }
        if (A.lag[k] > maxlag) maxlag = A.lag[k];
    }
    const int R = dsp_rows::ring_entries(maxlag);
    if (dsp_rows::lds_bytes(R) > LDS_BYTES_PER_CU / 2) return false;
    A.ring_entries = R;
    ch->rows_lds_bytes = dsp_rows::lds_bytes(R);
    A.trap_all_nan = dtr.ic[9];
    A.rr = dtr.fc[0];
    A.ll = dtr.fc[1];
    A.inv_rr = 1.0 / A.rr;
    A.inv_ll = 1.0 / A.ll;
    const int rise = tr->ip[0];
    A.rise_pow2 = (rise > 0 && (rise & (rise - 1)) == 0) ? 1 : 0;
    // reductions
    const int mm = tr->dst, tpt_reg = tr->io;
    if (tpt_reg >= 0) {
        if (!f32_or_const(tr->sp[0]) || tr->sp[2].kind != DSP_ARG_CONST) return false;
        if (tr->sp[0].kind == DSP_ARG_INPUT) {
            ch->rio_thr = tr->sp[0].index;
            A.thr_stride = io[ch->rio_thr].row_stride;
        } else {
            A.thr_const = (float)tr->sp[0].value;
        }
        const double walk = (double)(float)tr->sp[2].value;
        A.walk_nan = std::isnan(walk) ? 1 : 0;
        A.walk_frac = (!A.walk_nan && std::floor(walk) != walk) ? 1 : 0;
        const bool forward = !A.walk_nan && !A.walk_frac && (long long)walk == 1;
        const dsp_scalar_arg& t = tr->sp[1];
        if (t.kind == DSP_ARG_REG) {
            if (mm < 0 || (t.index != mm && t.index != mm + 1)) return false;
            A.tpt_use_min = t.index == mm ? 1 : 0;
            A.tpt_mode = forward ? 4 : 2;
        } else {
            if (!f32_or_const(t)) return false;
            if (t.kind == DSP_ARG_INPUT) {
                ch->rio_ts = t.index;
                A.ts_stride = io[ch->rio_ts].row_stride;
            } else {
                A.ts_const = (float)t.value;
            }
            A.tpt_mode = forward ? 3 : 1;
        }
    }
    for (const dsp_op* st : st_sc) {
        const int r = st->ip[0];
        if (io[st->io].dtype != DSP_F32) return false;
        if (mm >= 0 && r >= mm && r < mm + 4) {
            if (ch->rio_mm[r - mm] >= 0) return false;  // (one column per value)
            ch->rio_mm[r - mm] = st->io;
            A.out_mm_stride[r - mm] = io[st->io].row_stride;
        } else if (tpt_reg >= 0 && r == tpt_reg && ch->rio_tpt < 0) {
            ch->rio_tpt = st->io;
            A.out_tpt_stride = io[st->io].row_stride;
        } else {
            return false;
        }
    }
    if (dw) {
        const int level = dw->ip[0], outlen = slot_len[dw->dst];
        const dsp_io_desc& d = io[st_wf->io];
        if (level < 3 || level > 8 || len % (1 << level) != 0 || outlen != (len >> level) || outlen % 4 != 0 || d.row_stride % 4 != 0 ||
            d.offset % 4 != 0 || d.len != outlen)
            return false;
        A.dwt_level = level;
        A.dwt_part = dw->ip[1];
        A.dwt_stride = d.row_stride;
        ch->rio_dwt = st_wf->io;
    }
    // a walk backward from a known start on rows that are NaN-free or NaN from the first sample on (the LOAD's promise), and nothing else
    // asked for: what lies behind the start cannot change the answer -- the group stops there (the t0 trapezoid of the Ge recipes: half a row)
    bool any_mm = false;
    for (int k = 0; k < 4; ++k) any_mm |= ch->rio_mm[k] >= 0;
    A.stop_at_start = (A.tpt_mode == 1 && !any_mm && !dw && !has_pz && (ld.ip[2] & 1) && !A.walk_nan && !A.walk_frac && !A.trap_all_nan) ? 1 : 0;
    return true;
}


static int check_slot(const DevProgram& P, int s) { return s >= 0 && s < P.n_slots; }

static void mat2_mul(const long double* a, const long double* b, long double* o) {
    long double r[4] = {a[0] * b[0] + a[1] * b[2], a[0] * b[1] + a[1] * b[3], a[2] * b[0] + a[3] * b[2], a[2] * b[1] + a[3] * b[3]};
    memcpy(o, r, sizeof r);
}

// lag geometry shared by the three trapezoids (ic/fc layout documented in dsp_vm.hip)
static int setup_trap(DevOp& d, int kind_opcode, int rise, int flat, int fall, int len, int C) {
    if (rise < 0) return DSP_E_TRAP_RISE;
    if (flat < 0) return DSP_E_TRAP_FLAT;
    int L[3];
    if (kind_opcode == DSP_OP_ASYM_TRAP) {
        if (fall < 0) return DSP_E_TRAP_FALL;
        if ((int64_t)rise + flat + fall > len) return DSP_E_TRAP_WIDE;
        if (len > 0 && (rise == 0 || (fall == 0 && rise + flat < len))) return DSP_E_ZERODIV;
        L[0] = rise;
        L[1] = rise + flat;
        L[2] = rise + flat + fall;
    } else {
        if (2 * (int64_t)rise + flat > len) return DSP_E_TRAP_WIDE;
        if (kind_opcode == DSP_OP_TRAP_NORM && len > 0 && rise == 0) return DSP_E_ZERODIV;
        L[0] = rise;
        L[1] = rise + flat;
        L[2] = 2 * rise + flat;
    }
    for (int k = 0; k < 3; ++k) {
        d.ic[k] = L[k];
        d.ic[3 + k] = L[k] / C;
        d.ic[6 + k] = L[k] % C;
    }
    // trap_filter with rise == 0 reads w_out[-1] (the NaN fill) in its first step: the whole output is NaN
    d.ic[9] = (kind_opcode == DSP_OP_TRAP_FILTER && rise == 0) ? 1 : 0;
    d.ic[10] = (rise > 0 && (rise & (rise - 1)) == 0) ? 1 : 0;  // rise is a power of two: x / rise == x * (1 / rise), exactly
    d.fc[0] = (double)rise;
    d.fc[1] = (double)fall;
    return DSP_OK;
}

// waveform slots an op reads or writes (for the lifetime analysis of the LDS packing)
static int op_slots(const dsp_op& o, int out[4]) {
    switch (o.opcode) {
        case DSP_OP_LOAD: out[0] = o.dst; return 1;
        case DSP_OP_STORE:
        case DSP_OP_TRAP_PICKOFF:
        case DSP_OP_TRAP_REDUCE:
        case DSP_OP_PICKOFF:
        case DSP_OP_TIME_POINT_THRESH:
        case DSP_OP_INTERP_TIME_POINT_THRESH:
        case DSP_OP_MEAN_BELOW:
        case DSP_OP_TRAP_WINDOW_PICKOFF:
        case DSP_OP_MIN_MAX:
        case DSP_OP_LINEAR_SLOPE_FIT:
        case DSP_OP_AMAX:
        case DSP_OP_CONVOLVE_AMAX: out[0] = o.src; return 1;
        case DSP_OP_BL_SUBTRACT:
        case DSP_OP_MIN_MAX_NORM:
        case DSP_OP_POLE_ZERO:
        case DSP_OP_DOUBLE_POLE_ZERO:
        case DSP_OP_TRAP_FILTER:
        case DSP_OP_TRAP_NORM:
        case DSP_OP_ASYM_TRAP:
        case DSP_OP_COPY:
        case DSP_OP_WINDOWER:
        case DSP_OP_AVG_CURRENT:
        case DSP_OP_UPSAMPLER:
        case DSP_OP_PSD:
        case DSP_OP_FFT:
        case DSP_OP_SORT:
        case DSP_OP_INTERP_UPSAMPLE:
        case DSP_OP_REFLECTED_CONVOLVE:
        case DSP_OP_RC_CR2:
        case DSP_OP_LOG_CHECK:
        case DSP_OP_POLY_FIT:
        case DSP_OP_INL_CORRECTION:
        case DSP_OP_WF_ALIGNMENT:
        case DSP_OP_WF_CORRECTION:
        case DSP_OP_CONVOLVE: out[0] = o.src; out[1] = o.dst; return 2;
        case DSP_OP_WF_CENTROID:
        case DSP_OP_SVM_PREDICT: out[0] = o.src; return 1;
        case DSP_OP_POLY_DIFF:
        case DSP_OP_POLY_EXP_RMS: out[0] = o.src; out[1] = o.ip[0]; return 2;
        case DSP_OP_NORMALISE: out[0] = o.src; return 1;
        case DSP_OP_DENSE:
            out[0] = o.src;
            if (o.ip[3] == 0) return 1;  // (the classification form: dst is a scalar register)
            out[1] = o.dst;
            return 2;
        case DSP_OP_DWT_HAAR: out[0] = o.src; out[1] = o.dst; out[2] = o.ip[2]; return 3;
        case DSP_OP_MULTI_EXTREMA: out[0] = o.src; out[1] = o.dst; out[2] = o.ip[1]; return 3;
        case DSP_OP_BI_LEVEL_ZERO_CROSSING:
        case DSP_OP_PEAK_SNR_THRESHOLD:
        case DSP_OP_MULTI_A_FILTER:
        case DSP_OP_HISTOGRAM: out[0] = o.src; out[1] = o.dst; out[2] = o.ip[0]; return 3;
        case DSP_OP_HISTOGRAM_STATS: out[0] = o.src; out[1] = o.ip[0]; return 2;
        case DSP_OP_MULTI_TIME_POINT_THRESH:
            out[0] = o.src;
            out[1] = o.dst;
            if (o.ip[1] >= 0) {
                out[2] = o.ip[1];
                return 3;
            }
            return 2;
        case DSP_OP_TIME_OVER_THRESHOLD: out[0] = o.src; return 1;
        case DSP_OP_MOVING_WINDOW_MULTI:
            out[0] = o.src;
            out[1] = o.dst;
            if (o.ip[1] > 1 || o.ip[3] == 1) {
                out[2] = o.ip[2];
                return 3;
            }
            return 2;
        case DSP_OP_ELEMENTWISE: {
            int n = 0;
            out[n++] = o.dst;
            if (o.src >= 0) out[n++] = o.src;
            if (o.ip[1] >= 0) out[n++] = o.ip[1];
            if (o.ip[2] >= 0) out[n++] = o.ip[2];
            return n;
        }
        default: return 0;  // scalar ops
    }
}


static int check_call(PlanCtx& c) {
    const int n_ops = c.n_ops, n_io = c.n_io, n_slots = c.n_slots, n_sregs = c.n_sregs, compute_dtype = c.compute_dtype;
    if (!c.ops || !c.ch || n_ops <= 0 || n_ops > DSP_MAX_OPS) return fail(DSP_ERR_ARG, "n_ops=%d out of range (1..%d)", n_ops, DSP_MAX_OPS);
    if (n_io < 0 || n_io > DSP_MAX_IO) return fail(DSP_ERR_ARG, "n_io=%d out of range", n_io);
    if (n_slots < 0 || n_slots > DSP_MAX_SLOTS) return fail(DSP_ERR_ARG, "n_slots=%d out of range", n_slots);
    if (n_sregs < 0 || n_sregs > DSP_MAX_SREGS) return fail(DSP_ERR_ARG, "n_sregs=%d out of range", n_sregs);
    if (compute_dtype != DSP_F32 && compute_dtype != DSP_F64 && compute_dtype != DSP_I64)
        return fail(DSP_ERR_ARG, "compute_dtype must be DSP_F32, DSP_F64 or DSP_I64");
    c.i64 = compute_dtype == DSP_I64;  // an integer program of per-event values (dspeed_hip.h): 64-bit integer registers
    c.esz = compute_dtype == DSP_F32 ? 4 : 8;
    c.f64 = compute_dtype == DSP_F64;
    if (c.i64) {
        if (n_slots != 0) return fail(DSP_ERR_ARG, "an integer program (DSP_I64) has no waveform slots");
        for (int i = 0; i < n_ops; ++i)
            if (c.ops[i].opcode != DSP_OP_SCALAR_FUNC && c.ops[i].opcode != DSP_OP_STORE_SCALAR)
                return fail(DSP_ERR_ARG, "op %d: an integer program (DSP_I64) holds SCALAR_FUNC and STORE_SCALAR ops only", i);
    }

    DevProgram& P = c.ch->host;
    P.n_ops = n_ops;
    P.n_slots = n_slots;
    P.n_io = n_io;
    P.n_sregs = n_sregs;
    c.ch->f64 = c.f64;
    c.ch->i64 = c.i64;
    for (const KernelOnlyRoute& r : kernel_only_routes)
        for (int i = 0; i < n_ops && !c.only; ++i)
            for (const int opcode : r.opcodes)
                if (opcode != 0 && c.ops[i].opcode == opcode) c.only = &r;
    return DSP_OK;
}

// ---- LDS layout: [guard 2*pitch][slot 64*pitch][tail 8] per slot, then the scalar registers
// FIR inputs are laid out linearly (no chunk pad): a slot qualifies when a CONVOLVE reads it and everything else that touches
// it is layout-agnostic (load, store, copy, bl_subtract); the chunk-serial filters keep the padded, conflict-free layout
static void choose_linear_slots(PlanCtx& c) {
    for (int s = 0; s < c.n_slots; ++s) {
        bool fir_in = false, only_plain = true;
        for (int i = 0; i < c.n_ops; ++i) {
            const dsp_op& o = c.ops[i];
            int touched[4];
            const int nt = op_slots(o, touched);
            bool uses = false;
            for (int k = 0; k < nt; ++k) uses |= touched[k] == s;
            if (!uses) continue;
            const bool conv = o.opcode == DSP_OP_CONVOLVE || o.opcode == DSP_OP_CONVOLVE_AMAX;
            const bool reads = o.opcode != DSP_OP_LOAD && o.src == s;
            const bool writes = o.dst == s && (o.opcode == DSP_OP_LOAD || nt >= 2);  // (ELEMENTWISE: dst is touched[0], nt >= 2)  // (one-slot ops other than LOAD only read)
            if (conv && reads) fir_in = true;
            const bool plain = o.opcode == DSP_OP_LOAD || o.opcode == DSP_OP_STORE || o.opcode == DSP_OP_COPY ||
                               o.opcode == DSP_OP_BL_SUBTRACT || o.opcode == DSP_OP_MIN_MAX_NORM || (conv && reads && !writes);
            if (!plain) only_plain = false;
        }
        c.linear[s] = fir_in && only_plain;
    }
}

// first .. last op that touches each slot (a slot nothing touches: pack_lds keeps it alive throughout)
static void slot_lifetimes(PlanCtx& c) {
    for (int s = 0; s < c.n_slots; ++s) {
        c.first_op[s] = c.n_ops;
        c.last_op[s] = -1;
    }
    for (int i = 0; i < c.n_ops; ++i) {
        int touched[4];
        const int nt = op_slots(c.ops[i], touched);
        for (int k = 0; k < nt; ++k) {
            const int s = touched[k];
            if (s < 0 || s >= c.n_slots) continue;  // (rejected by the op checks of lower_ops)
            if (i < c.first_op[s]) c.first_op[s] = i;
            if (i > c.last_op[s]) c.last_op[s] = i;
        }
    }
}

// Slots whose lifetimes (first .. last op that touches them) do not overlap share LDS: the ICPC recipe has 14 waveform variables
// and at most four alive at a time.  Interval packing, first fit by first use; a slot that shares its region gets a
// DSP_OP_INTERNAL_ZERO in front of its first op (guards must read 0, pads finite -- also for the next row, which finds the region
// as the last tenant of the previous row left it).  Behind the slots: the register file and the scratch area.
static int pack_lds(PlanCtx& c) {
    ChainPlan* ch = c.ch;
    DevProgram& P = ch->host;
    const dsp_op* ops = c.ops;
    const dsp_io_desc* io = c.io;
    const int n_ops = c.n_ops, n_io = c.n_io, n_slots = c.n_slots;
    int *first_op = c.first_op, *last_op = c.last_op, *foot = c.foot, *base = c.base;
    for (int s = 0; s < n_slots; ++s) {
        const int len = c.slot_len[s];
        if (len <= 0) return fail(DSP_ERR_ARG, "slot %d has length %d", s, len);
        // (40 000 float32 samples fill a CU's LDS; the bound keeps the layout arithmetic below -- and the kernels' index -> (lane, offset)
        // split, exact for indices under 2^20 -- inside int)
        if (len > (1 << 20)) return fail(DSP_ERR_TOO_LONG, "slot %d: %d samples; a waveform variable lives in LDS (at most 2^20 samples are addressable)", s, len);
        int C = (len + 63) / 64;
        C = ((C + 15) / 16) * 16;
        DevSlot& d = P.slots[s];
        d.len = len;
        d.C = C;
        d.padw = c.linear[s] ? 0 : 1;
        d.pitch = C + d.padw;
        d.invC = 1.0f / (float)C;
        // a short FIR kernel (the t0 filter) in 'same' / 'full' mode reads up to m - 1 samples past either end of its input: give the
        // slot a zero tail long enough that those windows need no bounds checks (below sample 0 the guard serves)
        int fir_taps = 0;
        for (int i = 0; i < n_ops; ++i)
            if ((ops[i].opcode == DSP_OP_CONVOLVE || ops[i].opcode == DSP_OP_CONVOLVE_AMAX) && ops[i].src == s && ops[i].io >= 0 &&
                ops[i].io < n_io && io[ops[i].io].kind == DSP_IO_TAPS && io[ops[i].io].len <= 1024 && io[ops[i].io].len > fir_taps)
                fir_taps = io[ops[i].io].len;
        const int tail = 40 + (fir_taps ? fir_taps + 32 : 0);
        d.zero_below = 2 * d.pitch - 8;
        d.zero_above = (len == 64 * C) ? tail - 8 : 0;
        foot[s] = 2 * d.pitch + 64 * d.pitch + tail;  // guard, chunks, tail: the pipelined loops read up to 2 groups + 1 past the last chunk
        foot[s] = ((foot[s] + 3) / 4) * 4;          // (regions stay 16-byte aligned for the wide clears)
        if (last_op[s] < 0) {                        // never used: alive throughout, so nothing is placed on top of it
            first_op[s] = 0;
            last_op[s] = n_ops - 1;
        }
    }
    int order[DSP_MAX_SLOTS];
    for (int s = 0; s < n_slots; ++s) order[s] = s;
    std::stable_sort(order, order + n_slots, [&](int a, int b) { return first_op[a] < first_op[b]; });
    int cursor = 0;
    for (int oi = 0; oi < n_slots; ++oi) {
        const int s = order[oi];
        int at = 0;
        for (bool moved = true; moved;) {  // lowest offset where no slot alive at the same time lies
            moved = false;
            for (int oj = 0; oj < oi; ++oj) {
                const int t = order[oj];
                const bool alive_together = first_op[s] <= last_op[t] && first_op[t] <= last_op[s];
                if (alive_together && at < base[t] + foot[t] && base[t] < at + foot[s]) {
                    at = base[t] + foot[t];
                    moved = true;
                }
            }
        }
        base[s] = at;
        for (int oj = 0; oj < oi; ++oj) {
            const int t = order[oj];
            if (at < base[t] + foot[t] && base[t] < at + foot[s]) c.shares[s] = c.shares[t] = true;
        }
        P.slots[s].off = at + 2 * P.slots[s].pitch;
        if (at + foot[s] > cursor) cursor = at + foot[s];
    }
    P.sreg_off = cursor;
    cursor += ((c.n_sregs + 7) / 8) * 8 + 8;
    cursor = ((cursor + 3) / 4) * 4;
    P.scratch_off = cursor;
    cursor += DSP_SCRATCH_ELEMS;
    P.lds_elems_per_wave = cursor;
    ch->lds_bytes_per_wave = cursor * c.esz;
    if (ch->lds_bytes_per_wave > LDS_BYTES_PER_CU && !c.only)  // (MULTI_EXTREMA, HISTOGRAM, the threshold ops: their kernels stream the row through registers, no row lives in LDS; PSD, FFT, SORT, INTERP_UPSAMPLE, NORMALISE, DENSE, REFLECTED_CONVOLVE: their own layout and limits; RC_CR2, BI_LEVEL_ZERO_CROSSING: a tile of 64 rows; PEAK_SNR_THRESHOLD, MULTI_A_FILTER: nothing in LDS; LOG_CHECK, POLY_FIT, POLY_DIFF, POLY_EXP_RMS: a tile of 64 rows; INL_CORRECTION, WF_CENTROID, WF_ALIGNMENT, WF_CORRECTION: nothing in LDS; SVM_PREDICT: its own layout and limits)
        return fail(DSP_ERR_TOO_LONG, "chain needs %d bytes of LDS per waveform; a CU has %d", ch->lds_bytes_per_wave, LDS_BYTES_PER_CU);
    return DSP_OK;
}

// wavefronts per workgroup (1..4): the size that fits the most wavefronts into a CU's LDS and register budget (25 KB per
// waveform: 3 per group and 2 groups = 6 wavefronts, where 4 per group would leave one group of 4); ties go to the larger group.
// Register budget: the VM without the FIR op and 3 wavefronts per SIMD = 12 per CU, everything else 2 per SIMD = 8 per CU.
static void pick_waves_per_block(PlanCtx& c) {
    ChainPlan* ch = c.ch;
    for (int i = 0; i < c.n_ops; ++i) ch->has_fir |= (c.ops[i].opcode == DSP_OP_CONVOLVE || c.ops[i].opcode == DSP_OP_CONVOLVE_AMAX);
    auto pick_wpb = [&](int cap_waves) {
        int best_w = 1, best_waves = 0;
        for (int w = 1; w <= 4; ++w) {
            int groups = LDS_BYTES_PER_CU / (w * ch->lds_bytes_per_wave);
            if (groups > cap_waves / w) groups = cap_waves / w;  // whole groups only
            const int waves = groups * w;
            if (groups >= 1 && waves >= best_waves) {
                best_waves = waves;
                best_w = w;
            }
        }
        return best_w;
    };
    int wpb = pick_wpb(ch->has_fir ? 8 : 12);
    ch->classic_wpb = pick_wpb(8);
    ch->waves_per_block = wpb;
    ch->host.waves_per_block = wpb;
}

// ---- I/O bindings
static int bind_io(PlanCtx& c) {
    const bool f64 = c.f64, i64 = c.i64;
    for (int k = 0; k < c.n_io; ++k) {
        const dsp_io_desc& a = c.io[k];
        DevIO& d = c.ch->host.io[k];
        const int es = elem_size(a.dtype);
        if (!es) return fail(DSP_ERR_ARG, "io %d: unknown dtype %d", k, a.dtype);
        if (a.kind < DSP_IO_WF_IN || a.kind > DSP_IO_TAPS) return fail(DSP_ERR_ARG, "io %d: unknown kind %d", k, a.kind);
        if (a.len <= 0 || a.offset < 0) return fail(DSP_ERR_ARG, "io %d: bad len/offset", k);
        // rows lie row_stride elements apart and hold offset + len elements (dspeed_hip.h; 0: one row / value for every event); the bounds
        // keep the address arithmetic of the kernels and of this file inside 64 / 32 bits
        if (a.row_stride < 0 || a.row_stride > ((int64_t)1 << 40) || a.offset > (1 << 28) || a.len > (1 << 28))
            return fail(DSP_ERR_ARG, "io %d: row_stride / offset / len out of range", k);
        if ((a.kind == DSP_IO_WF_IN || a.kind == DSP_IO_WF_OUT) && (a.row_stride != 0 || a.kind == DSP_IO_WF_OUT) && (int64_t)a.offset + a.len > a.row_stride)
            return fail(DSP_ERR_ARG, "io %d: rows of %lld elements do not hold offset %d + len %d", k, (long long)a.row_stride, a.offset, a.len);
        // which rows may feed which loop: NumPy's can_cast rule as ProcessorManager applies it (processing_chain.py:1565-1572)
        if (a.kind == DSP_IO_WF_IN && !f64 && (a.dtype == DSP_I32 || a.dtype == DSP_U32 || a.dtype == DSP_F64) &&
            !(c.only && c.only->route == DSP_ROUTE_ALIGN && a.dtype != DSP_F64))  // (inl_correction's loop if->f: the matcher sees to the rest)
            return fail(DSP_ERR_ARG, "io %d: int32/uint32/float64 rows select the float64 loop (compute_dtype DSP_F64)", k);
        const bool is_out = a.kind == DSP_IO_WF_OUT || a.kind == DSP_IO_SCALAR_OUT;
        if ((is_out || a.kind == DSP_IO_TAPS) && a.dtype != c.compute_dtype && !(is_out && a.dtype == DSP_BOOL) && !(i64 && a.kind == DSP_IO_SCALAR_OUT) &&
            !(c.only && (c.only->route == DSP_ROUTE_EXTREMA || c.only->route == DSP_ROUTE_PILEUP || c.only->route == DSP_ROUTE_PULSES) && a.kind == DSP_IO_SCALAR_OUT && a.dtype == DSP_U32) &&  // (the counts of MULTI_EXTREMA, BI_LEVEL_ZERO_CROSSING and PEAK_SNR_THRESHOLD: their matchers see to the rest)
            !(c.only && c.only->route == DSP_ROUTE_TAILFIT && a.kind == DSP_IO_TAPS && a.dtype == DSP_F64) &&  // (POLY_FIT's inverted matrix: float64 in both loops)
            !(c.only && c.only->route == DSP_ROUTE_SVM && (a.kind == DSP_IO_TAPS || a.kind == DSP_IO_WF_OUT) && a.dtype == DSP_F64))  // (SVM_PREDICT's model and decisions: float64 in both loops)
            return fail(DSP_ERR_ARG, "io %d: outputs have the chain's compute type or DSP_BOOL, taps the compute type", k);
        if ((a.dtype == DSP_BOOL || a.dtype == DSP_I64 || a.dtype == DSP_U64) && a.kind != DSP_IO_SCALAR_IN && a.kind != DSP_IO_SCALAR_OUT && !(a.dtype == DSP_BOOL && is_out))
            return fail(DSP_ERR_ARG, "io %d: DSP_BOOL / DSP_I64 / DSP_U64 are types of per-event columns (DSP_BOOL also of waveform outputs)", k);
        if (i64 && a.kind == DSP_IO_SCALAR_IN && (a.dtype == DSP_F32 || a.dtype == DSP_F64))
            return fail(DSP_ERR_ARG, "io %d: an integer program (DSP_I64) reads integer and DSP_BOOL columns", k);
        if (!i64 && is_out && (a.dtype == DSP_I64 || a.dtype == DSP_U64))
            return fail(DSP_ERR_ARG, "io %d: 64-bit integer outputs are written by integer programs (compute_dtype DSP_I64)", k);
        d.kind = a.kind;
        d.dtype = a.dtype;
        d.len = a.len;
        d.offset = a.offset;
        d.row_stride = a.row_stride;
        d.vec_ok = ((a.row_stride * es) % 16 == 0) && (((int64_t)a.offset * es) % 16 == 0);
    }
    return DSP_OK;
}

static bool need_io(const PlanCtx& c, const dsp_op& o, int kind) { return o.io >= 0 && o.io < c.n_io && c.io[o.io].kind == kind; }
// the float32 loop receives float32 scalars, the float64 loop float64 ones
static double op_const(const PlanCtx& c, const dsp_op& o, int k) { return c.f64 ? o.sp[k].value : (double)(float)o.sp[k].value; }

// DOUBLE_POLE_ZERO: the coefficients of pole_zero.py:168-174 and the scan matrices M^(C*2^d)
static int lower_double_pole_zero(const PlanCtx& c, int i, const dsp_op& o, DevOp& d) {
    const DevProgram& P = c.ch->host;
    const int32_t* slot_len = c.slot_len;
    if (!check_slot(P, o.src) || !check_slot(P, o.dst) || slot_len[o.src] != slot_len[o.dst])
        return fail(DSP_ERR_ARG, "op %d: bad DOUBLE_POLE_ZERO", i);
    bool per_event = false;
    for (int k = 0; k < 3; ++k) per_event |= o.sp[k].kind != DSP_ARG_CONST;
    if (per_event) {  // a time constant or the fraction per event: coefficients and scan matrices are formed on the device
        if (slot_len[o.src] <= 3) return fail(DSP_E_DPZ_SHORT, "%s", dsp_fatal_message(DSP_E_DPZ_SHORT));
        d.ic[1] = 1;
        return DSP_OK;
    }
    const double tau1 = op_const(c, o, 0), tau2 = op_const(c, o, 1), fr = op_const(c, o, 2);
    d.ic[0] = (std::isnan(tau1) || std::isnan(tau2) || std::isnan(fr)) ? 1 : 0;
    if (!d.ic[0] && slot_len[o.src] <= 3) return fail(DSP_E_DPZ_SHORT, "%s", dsp_fatal_message(DSP_E_DPZ_SHORT));
    if (slot_len[o.src] <= 3) d.ic[0] = 1;
    const double a = std::exp(-1.0 / tau1), b = std::exp(-1.0 / tau2);  // pole_zero.py:168-174
    const double den1 = ((fr * b - fr * a) - b) - 1.0;
    const double den2 = -1.0 * ((fr * b - fr * a) - b);
    const double num1 = -1.0 * (a + b);
    const double num2 = a * b;
    d.fc[0] = num1;
    d.fc[1] = num2;
    d.fc[2] = den1;
    d.fc[3] = den2;
    // M^(C*2^d), d = 0..5, M = [[-den1, -den2], [1, 0]]
    long double M[4] = {-(long double)den1, -(long double)den2, 1.0L, 0.0L}, Pw[4] = {1, 0, 0, 1};
    const int C = P.slots[o.src].C;
    long double base[4];
    memcpy(base, M, sizeof base);
    for (int e = C; e; e >>= 1) {  // Pw = M^C
        if (e & 1) mat2_mul(Pw, base, Pw);
        mat2_mul(base, base, base);
    }
    for (int dd = 0; dd < 6; ++dd) {
        for (int k = 0; k < 4; ++k) d.fc[4 + 4 * dd + k] = (double)Pw[k];
        mat2_mul(Pw, Pw, Pw);
    }
    return DSP_OK;
}

static int lower_moving_window(const PlanCtx& c, int i, const dsp_op& o, DevOp& d) {
    const DevProgram& P = c.ch->host;
    const int32_t* slot_len = c.slot_len;
    const bool in_place = o.ip[3] == 1;
    if (!check_slot(P, o.src) || !check_slot(P, o.dst) || (o.src == o.dst) != in_place || slot_len[o.src] != slot_len[o.dst])
        return fail(DSP_ERR_ARG, "op %d: bad MOVING_WINDOW_MULTI", i);
    if (o.sp[0].kind != DSP_ARG_CONST) return fail(DSP_ERR_UNSUPPORTED, "moving_window_multi: the window length must be a constant");
    const double length = op_const(c, o, 0);
    const int num = o.ip[1], n = slot_len[o.src];
    if (floor(length) != length) return fail(DSP_E_MW_LEN_INT, "%s", dsp_fatal_message(DSP_E_MW_LEN_INT));
    if ((long long)length < 0 || (long long)length >= n) return fail(DSP_E_MW_LEN_RANGE, "%s", dsp_fatal_message(DSP_E_MW_LEN_RANGE));
    if (num < 0) return fail(DSP_E_MW_NUM_NEG, "%s", dsp_fatal_message(DSP_E_MW_NUM_NEG));
    if (num > 0 && (long long)length == 0) return fail(DSP_E_ZERODIV, "%s", dsp_fatal_message(DSP_E_ZERODIV));
    // (the scratch may be the source itself when the number of windows is odd: the first pass goes source -> target, so the
    // source is free from the second pass on -- and is overwritten)
    if (in_place) {  // ip[2]: a side slot for the ends of the chunks, 64 lanes x (L | 1) elements; the window inside one chunk
        const long long Lw = (long long)length;
        if (!check_slot(P, o.ip[2]) || o.ip[2] == o.src || Lw > P.slots[o.src].C || 64 * (Lw | 1) > 64LL * P.slots[o.ip[2]].pitch)
            return fail(DSP_ERR_ARG, "op %d: MOVING_WINDOW_MULTI in place needs a window of at most %d samples and a side slot of 64 x window samples (ip[2])",
                        i, P.slots[o.src].C);
    } else
    if (num > 1 && (!check_slot(P, o.ip[2]) || (o.ip[2] == o.src && num % 2 == 0) || o.ip[2] == o.dst || slot_len[o.ip[2]] != n))
        return fail(DSP_ERR_ARG, "op %d: MOVING_WINDOW_MULTI with several windows needs a scratch slot of the same length (ip[2])", i);
    d.ic[0] = (int)length;
    d.ic[1] = num;
    d.ic[2] = o.ip[0];
    d.fc[0] = length;
    return DSP_OK;
}

static int lower_convolve(const PlanCtx& c, int i, const dsp_op& o, DevOp& d) {
    const DevProgram& P = c.ch->host;
    const int32_t* slot_len = c.slot_len;
    const dsp_io_desc* io = c.io;
    const bool fusedmax = o.opcode == DSP_OP_CONVOLVE_AMAX;
    if (!check_slot(P, o.src) || !need_io(c, o, DSP_IO_TAPS)) return fail(DSP_ERR_ARG, "op %d: bad CONVOLVE", i);
    if (fusedmax ? (o.dst < 0 || o.dst >= c.n_sregs || o.ip[2] <= 0) : (!check_slot(P, o.dst) || o.src == o.dst))
        return fail(DSP_ERR_ARG, "op %d: bad CONVOLVE destination", i);
    // ip[3] > 0: the kernel has ip[3] taps and the binding holds zeros after them (up to a multiple of the tap block, so the
    // blocked path covers every tap; the op falls back to the true length for a waveform with an infinity in it: 0 * inf)
    if (o.ip[3] < 0 || o.ip[3] > io[o.io].len) return fail(DSP_ERR_ARG, "op %d: CONVOLVE kernel length beyond its binding", i);
    const int m = o.ip[3] > 0 ? o.ip[3] : io[o.io].len;
    const int n = slot_len[o.src], p = fusedmax ? o.ip[2] : slot_len[o.dst], mode = o.ip[0];
    d.ic[1] = m;
    d.ic[6] = io[o.io].len;
    d.ic[2] = (o.ip[1] & 1) ? 1 : 0;  // caller found a NaN among the taps -> output NaN (convolutions.py:45-46)
    d.ic[5] = (o.ip[1] & 2) ? 1 : 0;  // ... an infinity: 0 * inf is NaN, so windows must not reach into the zero margins
    d.ic[3] = p;
    if (m > n) return fail(DSP_E_CONV_LONG, "%s", dsp_fatal_message(DSP_E_CONV_LONG));
    if (mode == 'f') {
        if (p != n + m - 1) return fail(DSP_E_CONV_OUTLEN, "Output waveform has length %d; expect %d", p, n + m - 1);
        d.ic[0] = 0;
    } else if (mode == 'v') {
        if (p != n - m + 1) return fail(DSP_E_CONV_OUTLEN, "Output waveform has length %d; expect %d", p, n - m + 1);
        d.ic[0] = m - 1;
    } else if (mode == 's') {
        if (p != n) return fail(DSP_E_CONV_OUTLEN, "Output waveform has length %d; expect %d", p, n);
        d.ic[0] = (m - 1) / 2;
    } else {
        return fail(DSP_E_CONV_MODE, "%s", dsp_fatal_message(DSP_E_CONV_MODE));
    }
    return DSP_OK;
}

// validates one op of the caller's program and fills the constants of its device op `d` (a copy of the op already)
static int lower_op(const PlanCtx& c, int i, const dsp_op& o, DevOp& d) {
    const DevProgram& P = c.ch->host;
    const dsp_io_desc* io = c.io;
    const int32_t* slot_len = c.slot_len;
    const int n_sregs = c.n_sregs;
    const bool f64 = c.f64, i64 = c.i64;
    switch (o.opcode) {
        case DSP_OP_LOAD:
            if (!check_slot(P, o.dst) || !need_io(c, o, DSP_IO_WF_IN)) return fail(DSP_ERR_ARG, "op %d: bad LOAD", i);
            if (io[o.io].len != slot_len[o.dst]) return fail(DSP_ERR_ARG, "op %d: LOAD length mismatch", i);
            if (o.ip[0] < 0 || o.ip[1] < 0 || o.ip[0] > io[o.io].offset || (int64_t)io[o.io].offset + io[o.io].len + o.ip[1] > io[o.io].row_stride)
                return fail(DSP_ERR_ARG, "op %d: LOAD screens samples outside the row (ip[0], ip[1])", i);
            break;
        case DSP_OP_STORE:
            if (!check_slot(P, o.src) || !need_io(c, o, DSP_IO_WF_OUT)) return fail(DSP_ERR_ARG, "op %d: bad STORE", i);
            if (io[o.io].len != slot_len[o.src]) return fail(DSP_ERR_ARG, "op %d: STORE length mismatch", i);
            break;
        case DSP_OP_STORE_SCALAR:
            if (!need_io(c, o, DSP_IO_SCALAR_OUT) || o.ip[0] < 0 || o.ip[0] >= n_sregs) return fail(DSP_ERR_ARG, "op %d: bad STORE_SCALAR", i);
            break;
        case DSP_OP_BL_SUBTRACT:
        case DSP_OP_MIN_MAX_NORM:
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || slot_len[o.src] != slot_len[o.dst])
                return fail(DSP_ERR_ARG, "op %d: bad element-wise op", i);
            break;
        case DSP_OP_POLE_ZERO: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || slot_len[o.src] != slot_len[o.dst])
                return fail(DSP_ERR_ARG, "op %d: bad POLE_ZERO", i);
            if (o.sp[0].kind != DSP_ARG_CONST) {  // one tau per event: the constant is formed on the device (op_pole_zero)
                d.ic[1] = 1;
                break;
            }
            const double tau = op_const(c, o, 0);
            d.ic[0] = std::isnan(tau) ? 1 : 0;
            d.fc[0] = std::exp(-1.0 / tau);  // pole_zero.py:60 -- float64 via libm, like numba's lowering
            break;
        }
        case DSP_OP_DOUBLE_POLE_ZERO: return lower_double_pole_zero(c, i, o, d);
        case DSP_OP_TRAP_FILTER:
        case DSP_OP_TRAP_NORM:
        case DSP_OP_ASYM_TRAP: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || o.src == o.dst || slot_len[o.src] != slot_len[o.dst])
                return fail(DSP_ERR_ARG, "op %d: bad trapezoid (source and destination slots must differ)", i);
            int rc = setup_trap(d, o.opcode, o.ip[0], o.ip[1], o.ip[2], slot_len[o.src], P.slots[o.src].C);
            if (rc) return fail(rc, "%s", dsp_fatal_message(rc));
            break;
        }
        case DSP_OP_TRAP_PICKOFF: {
            if (!check_slot(P, o.src) || o.dst < 0 || o.dst >= n_sregs) return fail(DSP_ERR_ARG, "op %d: bad TRAP_PICKOFF", i);
            if (o.ip[3] != DSP_OP_TRAP_FILTER && o.ip[3] != DSP_OP_TRAP_NORM && o.ip[3] != DSP_OP_ASYM_TRAP)
                return fail(DSP_ERR_ARG, "op %d: TRAP_PICKOFF ip[3] must name a trapezoid opcode", i);
            if (o.io == 's')
                return fail(DSP_ERR_UNSUPPORTED, "TRAP_PICKOFF cannot take mode 's' (the spline needs the whole filtered waveform): use TRAP_FILTER + PICKOFF");
            int rc = setup_trap(d, o.ip[3], o.ip[0], o.ip[1], o.ip[2], slot_len[o.src], P.slots[o.src].C);
            if (rc) return fail(rc, "%s", dsp_fatal_message(rc));
            break;
        }
        case DSP_OP_TRAP_REDUCE: {
            if (!check_slot(P, o.src) || (o.dst < 0 && o.io < 0) || (o.dst >= 0 && o.dst > n_sregs - 4) || o.io >= n_sregs)
                return fail(DSP_ERR_ARG, "op %d: bad TRAP_REDUCE", i);
            const int tk = o.ip[3] & 0xff, pk_mode = (o.ip[3] >> 8) & 0xff, pk_reg = ((o.ip[3] >> 16) & 0x3fff) - 1;
            if (tk != DSP_OP_TRAP_FILTER && tk != DSP_OP_TRAP_NORM && tk != DSP_OP_ASYM_TRAP)
                return fail(DSP_ERR_ARG, "op %d: TRAP_REDUCE ip[3] must name a trapezoid opcode", i);
            if (pk_reg >= n_sregs || (pk_reg >= 0 && (pk_mode == 0 || pk_mode == 's')) || (pk_reg < 0 && pk_mode != 0))
                return fail(DSP_ERR_ARG, "op %d: bad pick-off in TRAP_REDUCE (register %d, mode %d)", i, pk_reg, pk_mode);
            if (((o.ip[3] >> 30) & 1) && (o.dst < 0 || tk == DSP_OP_ASYM_TRAP))
                return fail(DSP_ERR_ARG, "op %d: TRAP_REDUCE amax-only needs the min_max registers and trap_filter / trap_norm", i);
            int rc = setup_trap(d, tk, o.ip[0], o.ip[1], o.ip[2], slot_len[o.src], P.slots[o.src].C);
            if (rc) return fail(rc, "%s", dsp_fatal_message(rc));
            break;
        }
        case DSP_OP_PICKOFF:
            if (!check_slot(P, o.src) || o.dst < 0 || o.dst >= n_sregs) return fail(DSP_ERR_ARG, "op %d: bad PICKOFF", i);
            if (o.ip[1] < 0 || o.ip[1] > 2) return fail(DSP_ERR_ARG, "op %d: PICKOFF ip[1] must be 0, 1 or 2", i);
            if (o.ip[1] == 2 && o.sp[1].kind != DSP_ARG_CONST) return fail(DSP_ERR_ARG, "op %d: PICKOFF ip[1] = 2 takes a constant default (sp[1])", i);
            if (o.ip[1] == 1 && (o.sp[0].kind != DSP_ARG_CONST || o.sp[0].value < 0 || o.sp[0].value >= slot_len[o.src] ||
                                 o.sp[0].value != std::floor(o.sp[0].value)))
                return fail(DSP_ERR_ARG, "op %d: PICKOFF of one sample (ip[1] = 1) needs a constant index inside the waveform", i);
            break;
        case DSP_OP_TIME_POINT_THRESH:
        case DSP_OP_INTERP_TIME_POINT_THRESH:
            if (!check_slot(P, o.src) || o.dst < 0 || o.dst >= n_sregs) return fail(DSP_ERR_ARG, "op %d: bad TIME_POINT_THRESH", i);
            break;
        case DSP_OP_MEAN_BELOW:
            if (!check_slot(P, o.src) || o.dst < 0 || o.dst >= n_sregs) return fail(DSP_ERR_ARG, "op %d: bad MEAN_BELOW", i);
            break;
        case DSP_OP_WINDOWER:
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || o.src == o.dst) return fail(DSP_ERR_ARG, "op %d: bad WINDOWER", i);
            if (slot_len[o.dst] >= slot_len[o.src]) return fail(DSP_E_WINDOW_LONG, "%s", dsp_fatal_message(DSP_E_WINDOW_LONG));
            break;
        case DSP_OP_AVG_CURRENT: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || o.src == o.dst) return fail(DSP_ERR_ARG, "op %d: bad AVG_CURRENT", i);
            if (o.sp[0].kind != DSP_ARG_CONST) return fail(DSP_ERR_UNSUPPORTED, "avg_current: the window length must be a constant");
            const double length = op_const(c, o, 0);
            const int n = slot_len[o.src];
            if (!(length >= 0) || !(length < (double)n)) return fail(DSP_E_AVGCUR_RANGE, "%s", dsp_fatal_message(DSP_E_AVGCUR_RANGE));
            const int L = (int)length;
            if (L <= 0 || slot_len[o.dst] != n - L)
                return fail(DSP_ERR_ARG, "avg_current: the output must hold len(w_in) - int(length) = %d samples (it holds %d)", n - L,
                            slot_len[o.dst]);
            d.ic[0] = L;
            d.fc[0] = length;
            break;
        }
        case DSP_OP_UPSAMPLER: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || o.src == o.dst) return fail(DSP_ERR_ARG, "op %d: bad UPSAMPLER", i);
            if (o.sp[0].kind != DSP_ARG_CONST) return fail(DSP_ERR_UNSUPPORTED, "upsampler: the factor must be a constant");
            const double up = op_const(c, o, 0);
            if (!(up > 0)) return fail(DSP_E_UPSAMPLE, "%s", dsp_fatal_message(DSP_E_UPSAMPLE));
            d.fc[0] = up;
            d.fc[1] = floor(up / 2.0);
            d.ic[0] = (int)up;
            break;
        }
        case DSP_OP_MOVING_WINDOW_MULTI: return lower_moving_window(c, i, o, d);
        case DSP_OP_TRAP_WINDOW_PICKOFF: {
            if (!check_slot(P, o.src) || o.dst < 0 || o.dst >= n_sregs) return fail(DSP_ERR_ARG, "op %d: bad TRAP_WINDOW_PICKOFF", i);
            const int rise = o.ip[0], flat = o.ip[1];
            if (rise < 0) return fail(DSP_E_TRAP_RISE, "%s", dsp_fatal_message(DSP_E_TRAP_RISE));
            if (flat < 0) return fail(DSP_E_TRAP_FLAT, "%s", dsp_fatal_message(DSP_E_TRAP_FLAT));
            if (2 * (long long)rise + flat > slot_len[o.src]) return fail(DSP_E_TRAP_WIDE, "%s", dsp_fatal_message(DSP_E_TRAP_WIDE));
            break;
        }
        case DSP_OP_MIN_MAX:
            if (!check_slot(P, o.src) || o.dst < 0 || o.dst > n_sregs - 4) return fail(DSP_ERR_ARG, "op %d: bad MIN_MAX", i);
            break;
        case DSP_OP_LINEAR_SLOPE_FIT: {
            if (!check_slot(P, o.src) || o.dst < 0 || o.dst > n_sregs - 4) return fail(DSP_ERR_ARG, "op %d: bad LINEAR_SLOPE_FIT", i);
            const int first = o.ip[0];
            if (first < 0 || first > slot_len[o.src]) return fail(DSP_ERR_ARG, "op %d: LINEAR_SLOPE_FIT slice out of range", i);
            const int count = o.ip[1] > 0 ? o.ip[1] : slot_len[o.src] - first;  // ip[1] == 0: to the end of the slot
            if (count < 0 || count > slot_len[o.src] - first) return fail(DSP_ERR_ARG, "op %d: LINEAR_SLOPE_FIT slice out of range", i);
            if (count < 2) return fail(DSP_E_ZERODIV, "%s", dsp_fatal_message(DSP_E_ZERODIV));  // the line fit's denominator
            d.ic[0] = first;
            d.ic[1] = count;
            break;
        }
        case DSP_OP_AMAX:
            if (!check_slot(P, o.src) || o.dst < 0 || o.dst >= n_sregs) return fail(DSP_ERR_ARG, "op %d: bad AMAX", i);
            break;
        case DSP_OP_MULTI_EXTREMA: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || !check_slot(P, o.ip[1]) || o.dst == o.src || o.ip[1] == o.src || o.dst == o.ip[1] ||
                slot_len[o.dst] != slot_len[o.ip[1]] || o.ip[2] < 0 || o.ip[2] > n_sregs - 2)
                return fail(DSP_ERR_ARG, "op %d: bad MULTI_EXTREMA (dst, ip[1]: two slots of one length for the lists; ip[2]: two registers for the counts)", i);
            // the reference's checks in its order (get_multi_local_extrema.py:126-131, 305-306), for everything that is a constant
            if (slot_len[o.dst] >= slot_len[o.src]) return fail(DSP_E_EXTREMA_LEN, "%s", dsp_fatal_message(DSP_E_EXTREMA_LEN));
            for (int k = 0; k < 2; ++k)
                if (o.sp[k].kind == DSP_ARG_CONST && op_const(c, o, k) < 0) return fail(DSP_E_EXTREMA_DELTA, "%s", dsp_fatal_message(DSP_E_EXTREMA_DELTA));
            if (o.ip[0] < 0 || o.ip[0] > 3) return fail(DSP_E_EXTREMA_DIR, "%s", dsp_fatal_message(DSP_E_EXTREMA_DIR));
            if (o.ip[0] == 2)
                return fail(DSP_ERR_UNSUPPORTED, "get_multi_local_extrema: search_direction 2 (extrema found in both directions) is not implemented: the reference's "
                                                 "branch reads the maxima with the minima's mask and defines no result to agree with");
            if (o.ip[0] == 3 && slot_len[o.dst] > DSP_EXTREMA_UNION_MAX)
                return fail(DSP_ERR_UNSUPPORTED, "get_multi_local_extrema: search_direction 3 takes lists of at most %d entries (%d asked for)", DSP_EXTREMA_UNION_MAX,
                            slot_len[o.dst]);
            break;
        }
        case DSP_OP_HISTOGRAM: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || !check_slot(P, o.ip[0]) || o.dst == o.src || o.ip[0] == o.src || o.dst == o.ip[0])
                return fail(DSP_ERR_ARG, "op %d: bad HISTOGRAM (dst: the slot of the weights, ip[0]: the slot of the borders)", i);
            if (o.ip[1] < 0) return fail(DSP_ERR_ARG, "op %d: HISTOGRAM ip[1] (the most workgroups the rows are dealt out to, 0: no cap of the program's) is negative", i);
            if (slot_len[o.ip[0]] != slot_len[o.dst] + 1) return fail(DSP_E_HIST_LEN, "%s", dsp_fatal_message(DSP_E_HIST_LEN));
            if (slot_len[o.dst] > DSP_HIST_MAX_BINS)
                return fail(DSP_ERR_UNSUPPORTED, "histogram: at most %d bins (%d asked for): a wavefront keeps a counter per bin in LDS", DSP_HIST_MAX_BINS, slot_len[o.dst]);
            if (!f64 && slot_len[o.src] > (1 << 24))
                return fail(DSP_ERR_UNSUPPORTED, "histogram: the float32 loop takes rows of at most 2^24 samples (%d): a weight counts them exactly", slot_len[o.src]);
            break;
        }
        case DSP_OP_HISTOGRAM_STATS: {
            if (!check_slot(P, o.src) || !check_slot(P, o.ip[0]) || o.src == o.ip[0] || o.ip[1] < 0 || o.ip[1] > n_sregs - 3)
                return fail(DSP_ERR_ARG, "op %d: bad HISTOGRAM_STATS (src, ip[0]: the slots of weights and edges; ip[1]: three registers for mode, max, fwhm)", i);
            if (slot_len[o.ip[0]] != slot_len[o.src] + 1) return fail(DSP_E_HIST_STATS_LEN, "%s", dsp_fatal_message(DSP_E_HIST_STATS_LEN));
            if (slot_len[o.src] > DSP_HIST_MAX_BINS)
                return fail(DSP_ERR_UNSUPPORTED, "histogram_stats: at most %d bins (%d given)", DSP_HIST_MAX_BINS, slot_len[o.src]);
            break;
        }
        case DSP_OP_MULTI_TIME_POINT_THRESH: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || o.dst == o.src || (o.ip[1] >= 0 && (!check_slot(P, o.ip[1]) || o.ip[1] == o.src || o.ip[1] == o.dst)))
                return fail(DSP_ERR_ARG, "op %d: bad MULTI_TIME_POINT_THRESH (dst: the slot of t_out; ip[1]: the slot of a list of thresholds per row, or < 0: one list, the op's DSP_IO_TAPS binding)", i);
            if (o.ip[1] >= 0 ? slot_len[o.ip[1]] != slot_len[o.dst] : (need_io(c, o, DSP_IO_TAPS) && io[o.io].len != slot_len[o.dst]))
                return fail(DSP_ERR_ARG, "op %d: MULTI_TIME_POINT_THRESH writes a time per threshold (%d thresholds, %d times)", i,
                            o.ip[1] >= 0 ? slot_len[o.ip[1]] : io[o.io].len, slot_len[o.dst]);
            // polarity and mode: constants, checked for every row (the reference raises only on rows that get that far)
            if (o.sp[1].kind != DSP_ARG_CONST)
                return fail(DSP_ERR_UNSUPPORTED, "multi_time_point_thresh: the polarity is a constant of the program, not a per-event value");
            if (!(op_const(c, o, 1) > 0) && !(op_const(c, o, 1) < 0)) return fail(DSP_E_MTPT_POLARITY, "%s", dsp_fatal_message(DSP_E_MTPT_POLARITY));
            if (o.ip[0] <= 0 || o.ip[0] > 127 || !strchr("iafbcrnl", o.ip[0])) return fail(DSP_E_MTPT_MODE, "%s", dsp_fatal_message(DSP_E_MTPT_MODE));
            if (slot_len[o.dst] > DSP_THRESH_MAX)
                return fail(DSP_ERR_UNSUPPORTED, "multi_time_point_thresh: at most %d thresholds (%d given): a wavefront keeps one per lane", DSP_THRESH_MAX, slot_len[o.dst]);
            if (slot_len[o.src] < 2)
                return fail(DSP_ERR_UNSUPPORTED, "multi_time_point_thresh: rows of at least 2 samples (%d): the walks compare neighbours", slot_len[o.src]);
            if (!f64 && slot_len[o.src] > (1 << 24))
                return fail(DSP_ERR_UNSUPPORTED, "multi_time_point_thresh: the float32 loop takes rows of at most 2^24 samples (%d): a time counts them exactly", slot_len[o.src]);
            break;
        }
        case DSP_OP_TIME_OVER_THRESHOLD: {
            if (!check_slot(P, o.src) || o.dst < 0 || o.dst >= n_sregs)
                return fail(DSP_ERR_ARG, "op %d: bad TIME_OVER_THRESHOLD (src: the slot of the row; dst: the register of the count)", i);
            if (!f64 && slot_len[o.src] > (1 << 24))
                return fail(DSP_ERR_UNSUPPORTED, "time_over_threshold: the float32 loop takes rows of at most 2^24 samples (%d): the count is exact", slot_len[o.src]);
            break;
        }
        case DSP_OP_PSD:
        case DSP_OP_FFT: {
            const bool cplx = o.opcode == DSP_OP_FFT;
            const char* name = cplx ? "fft" : "psd";
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || o.dst == o.src)
                return fail(DSP_ERR_ARG, "op %d: bad %s (src: the slot of the row; dst: the slot of the spectrum%s)", i, cplx ? "FFT" : "PSD",
                            cplx ? ", (re, im) pairs" : "");
            const int n = slot_len[o.src], m = n / 2 + 1;
            // the reference's check, first (fft.py:39-40, 119-120)
            if (slot_len[o.dst] != (cplx ? 2 * m : m)) return fail(cplx ? DSP_E_FFT_LEN : DSP_E_PSD_LEN, "Size of %s must be len(w_in)//2+1 = %d", name, m);
            const int pow2_max = DSP_SPECTRUM_F32_POW2_MAX / (f64 ? 2 : 1), any_max = DSP_SPECTRUM_F32_ANY_MAX / (f64 ? 2 : 1);
            if (dsp_spectrum::pow2(n) ? n > pow2_max : n > any_max)
                return fail(DSP_ERR_UNSUPPORTED, "%s: the %s loop takes rows of a power of two up to %d samples and of any other length up to %d (%d given): a row's transform lives in 64 KiB of LDS",
                            name, f64 ? "float64" : "float32", pow2_max, any_max, n);
            break;
        }
        case DSP_OP_SORT: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || o.dst == o.src)
                return fail(DSP_ERR_ARG, "op %d: bad SORT (src: the slot of the row; dst: another slot, for the sorted row)", i);
            const int n = slot_len[o.src], n_max = DSP_SORT_F32_MAX / (f64 ? 2 : 1);
            if (slot_len[o.dst] != n) return fail(DSP_ERR_ARG, "op %d: SORT: the sorted row has the row's length (%d; %d given)", i, n, slot_len[o.dst]);
            if (n > n_max)
                return fail(DSP_ERR_UNSUPPORTED, "sort: rows of up to %d samples in the float32 loop and %d in the float64 loop (%d given): a row's keys live in 64 KiB of LDS",
                            DSP_SORT_F32_MAX, DSP_SORT_F32_MAX / 2, n);
            break;
        }
        case DSP_OP_INTERP_UPSAMPLE: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || o.dst == o.src)
                return fail(DSP_ERR_ARG, "op %d: bad INTERP_UPSAMPLE (src: the slot of the row; dst: another slot, for the resampled row; ip[0]: the mode)", i);
            const int n = slot_len[o.src], m = slot_len[o.dst], mode = o.ip[0], es = f64 ? 8 : 4;
            static_assert(dsp_interp::max_len('l', 4) == DSP_INTERP_F32_MAX && dsp_interp::max_len('l', 8) == DSP_INTERP_F32_MAX / 2 &&
                              dsp_interp::max_len('s', 4) == DSP_INTERP_SPLINE_F32_MAX && dsp_interp::max_len('s', 8) == DSP_INTERP_SPLINE_F64_MAX,
                          "the limits the texts name are the geometry's");
            if (n < 1 || m < 1) return fail(DSP_ERR_ARG, "op %d: INTERP_UPSAMPLE: the row and the resampled row hold at least one sample (%d and %d given)", i, n, m);
            if (!dsp_interp::mode_ok(mode)) return fail(DSP_ERR_ARG, "interpolating_upsampler: Unrecognized interpolation mode (%d)", mode);
            if (mode == 'i' && m % n != 0)
                return fail(DSP_ERR_ARG, "interpolating_upsampler requires len(w_out) to be an integer multiple of len(w_in) for mode 'i' (%d and %d given)", m, n);
            if (mode == 'h' && n < 2)
                return fail(DSP_ERR_UNSUPPORTED, "interpolating_upsampler: mode 'h' takes rows of at least 2 samples (%d given): the reference reads an unbound variable there", n);
            if (n > dsp_interp::max_len(mode, es)) {
                if (mode == 's')
                    return fail(DSP_ERR_UNSUPPORTED, "interpolating_upsampler: mode 's' takes rows of up to %d samples in the float32 loop and %d in the float64 loop (%d given): "
                                "the row and its second derivatives live in 64 KiB of LDS", DSP_INTERP_SPLINE_F32_MAX, DSP_INTERP_SPLINE_F64_MAX, n);
                return fail(DSP_ERR_UNSUPPORTED, "interpolating_upsampler: rows of up to %d samples in the float32 loop and %d in the float64 loop (%d given): a row lives in 64 KiB of LDS",
                            DSP_INTERP_F32_MAX, DSP_INTERP_F32_MAX / 2, n);
            }
            break;
        }
        case DSP_OP_NORMALISE: {
            if (!check_slot(P, o.src) || o.dst != o.src)
                return fail(DSP_ERR_ARG, "op %d: bad NORMALISE (src = dst: the slot of the row, normalised in place)", i);
            const int n = slot_len[o.src];
            if (n > DSP_DENSE_N_MAX)
                return fail(DSP_ERR_UNSUPPORTED, "normalisation_layer: " DSP_DENSE_LIMITS_TEXT " (n = %d given)", DSP_DENSE_N_MAX, DSP_DENSE_M_MAX, n);
            if (!need_io(c, o, DSP_IO_TAPS) || io[o.io].len != n || o.ip[0] < 0 || o.ip[0] >= c.n_io || io[o.ip[0]].kind != DSP_IO_TAPS || io[o.ip[0]].len != n)
                return fail(DSP_ERR_ARG, "normalisation_layer: means (io) and variances (ip[0]) are DSP_IO_TAPS bindings of len(x_in) = %d values", n);
            break;
        }
        case DSP_OP_DENSE: {
            const bool classify = o.ip[3] == 0;
            if (!check_slot(P, o.src) || (classify ? (o.dst < 0 || o.dst >= n_sregs) : (!check_slot(P, o.dst) || o.dst == o.src)))
                return fail(DSP_ERR_ARG, "op %d: bad DENSE (src: the slot of the row; dst: another slot, of ip[3] = m samples, or with ip[3] = 0 a scalar register)", i);
            static_assert(dsp_dense::N_MAX == DSP_DENSE_N_MAX && dsp_dense::M_MAX == DSP_DENSE_M_MAX, "the limits the text names are the geometry's");
            const int n = slot_len[o.src], m = classify ? 1 : o.ip[3];
            if (o.ip[2] != n || (!classify && (m < 1 || slot_len[o.dst] != m)))
                return fail(DSP_ERR_ARG, "op %d: DENSE: ip[2] is the length of the row (%d), ip[3] that of the output slot or 0 (%d and %d given)", i, n, o.ip[2], o.ip[3]);
            if (n > DSP_DENSE_N_MAX || m > DSP_DENSE_M_MAX)
                return fail(DSP_ERR_UNSUPPORTED, "dense_layer: " DSP_DENSE_LIMITS_TEXT " (n = %d, m = %d given)", DSP_DENSE_N_MAX, DSP_DENSE_M_MAX, n, m);
            if (!need_io(c, o, DSP_IO_TAPS) || (int64_t)io[o.io].len != (int64_t)n * m)
                return fail(DSP_ERR_ARG, "dense_layer: the weights (io) are a DSP_IO_TAPS binding of n * m = %d * %d values, row-major", n, m);
            if (o.ip[1] >= 0 && (o.ip[1] >= c.n_io || io[o.ip[1]].kind != DSP_IO_TAPS || io[o.ip[1]].len != m))
                return fail(DSP_ERR_ARG, "dense_layer: the bias (ip[1]) is a DSP_IO_TAPS binding of m = %d values, or -1", m);
            break;
        }
        case DSP_OP_SVM_PREDICT: {
            if (!check_slot(P, o.src) || o.dst < 0 || o.dst >= n_sregs)
                return fail(DSP_ERR_ARG, "op %d: bad SVM_PREDICT (src: the slot of the row; dst: the register of the label)", i);
            static_assert(dsp_svm::N_MAX == DSP_DENSE_N_MAX && dsp_svm::CLASSES_MAX == DSP_SVM_CLASSES_MAX, "the limits the text names are the geometry's");
            auto model = [&](int k) { return k >= 0 && k < c.n_io && io[k].kind == DSP_IO_TAPS && io[k].dtype == DSP_F64; };
            if (!model(o.io) || !model(o.ip[0]) || !model(o.ip[1]) || !model(o.ip[2]) || !model(o.ip[3]))
                return fail(DSP_ERR_ARG, "svm_predict: support vectors (io), their squared norms (ip[0]), D (ip[1]), intercepts (ip[2]) and classes (ip[3]) are DSP_IO_TAPS bindings of DSP_F64 in both loops");
            const int n = slot_len[o.src], k = io[o.ip[3]].len, n_sv = io[o.ip[0]].len;
            if (n > DSP_DENSE_N_MAX || k > DSP_SVM_CLASSES_MAX)
                return fail(DSP_ERR_UNSUPPORTED, "svm_predict: " DSP_SVM_LIMITS_TEXT " (n = %d, %d classes given)", DSP_DENSE_N_MAX, DSP_SVM_CLASSES_MAX, n, k);
            if (k < 2) return fail(DSP_ERR_ARG, "svm_predict: a model has at least 2 classes (%d given)", k);
            const int pairs = dsp_svm::pairs(k);
            if (io[o.ip[2]].len != pairs || (int64_t)io[o.io].len != (int64_t)n_sv * n || (int64_t)io[o.ip[1]].len != (int64_t)n_sv * pairs)
                return fail(DSP_ERR_ARG, "svm_predict: %d classes, %d support vectors and rows of %d samples take %d intercepts, %lld support-vector samples and %lld coefficients (%d, %d and %d given)",
                            k, n_sv, n, pairs, (long long)n_sv * n, (long long)n_sv * pairs, io[o.ip[2]].len, io[o.io].len, io[o.ip[1]].len);
            if (o.sp[0].kind != DSP_ARG_CONST || o.sp[1].kind != DSP_ARG_CONST || o.sp[2].kind != DSP_ARG_CONST || (o.sp[1].value != 0.0 && o.sp[1].value != 1.0))
                return fail(DSP_ERR_ARG, "svm_predict: gamma (sp[0]), the kernel function (sp[1]: 0 rbf, 1 linear) and the decisions' binding (sp[2]) are constants of the program");
            const double dec = o.sp[2].value;
            if (dec != -1.0 && !(dec >= 0 && dec < c.n_io && dec == (double)(int)dec && io[(int)dec].kind == DSP_IO_WF_OUT && io[(int)dec].dtype == DSP_F64 && io[(int)dec].len == pairs))
                return fail(DSP_ERR_ARG, "svm_predict: the decisions (sp[2]) are a DSP_IO_WF_OUT binding of P = %d DSP_F64 values a row, or -1", pairs);
            break;
        }
        case DSP_OP_REFLECTED_CONVOLVE: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || o.dst == o.src || !need_io(c, o, DSP_IO_TAPS))
                return fail(DSP_ERR_ARG, "op %d: bad REFLECTED_CONVOLVE (src: the slot of the row; dst: another slot, for the filtered row; io: the kernel, a DSP_IO_TAPS binding)", i);
            static_assert(dsp_reflect::F32_MAX == DSP_REFLECT_F32_MAX && dsp_reflect::F64_MAX == DSP_REFLECT_F64_MAX, "the limits the text names are the geometry's");
            const int n = slot_len[o.src], m = io[o.io].len;
            if (n < 1 || m < 1) return fail(DSP_ERR_ARG, "op %d: REFLECTED_CONVOLVE: the row and the kernel hold at least one sample (%d and %d given)", i, n, m);
            if (m > n) return fail(DSP_ERR_ARG, "The filter is longer than the input waveform (%d taps, %d samples)", m, n);
            if (slot_len[o.dst] != n)
                return fail(DSP_ERR_ARG, "reflected_convolve_wf: the output has the length of the input (len(w_in) = %d, len(w_out) = %d)", n, slot_len[o.dst]);
            if (!dsp_reflect::fits(n, m, f64 ? 8 : 4))
                return fail(DSP_ERR_UNSUPPORTED, "reflected_convolve_wf: " DSP_REFLECT_LIMITS_TEXT " (len(w_in) = %d, len(kernel) = %d given): a row and its mirrored margins live in 64 KiB of LDS",
                            DSP_REFLECT_F32_MAX, DSP_REFLECT_F64_MAX, n, m);
            break;
        }
        case DSP_OP_RC_CR2: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || o.dst == o.src)
                return fail(DSP_ERR_ARG, "op %d: bad RC_CR2 (src: the slot of the row; dst: another slot, for the filtered row; sp[0]: t_tau)", i);
            if (o.sp[0].kind != DSP_ARG_CONST)
                return fail(DSP_ERR_UNSUPPORTED, "rc_cr2: t_tau is a constant of the program, not a per-event value: its coefficients are formed on the host");
            if (slot_len[o.src] < dsp_pileup::MIN_FILTER_LEN) return fail(DSP_E_DPZ_SHORT, "%s", dsp_fatal_message(DSP_E_DPZ_SHORT));
            if (slot_len[o.dst] != slot_len[o.src])
                return fail(DSP_ERR_ARG, "rc_cr2: the output has the length of the input (len(w_in) = %d, len(w_out) = %d)", slot_len[o.src], slot_len[o.dst]);
            break;
        }
        case DSP_OP_BI_LEVEL_ZERO_CROSSING: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || !check_slot(P, o.ip[0]) || o.dst == o.src || o.ip[0] == o.src || o.dst == o.ip[0] || o.ip[1] < 0 ||
                o.ip[1] >= n_sregs)
                return fail(DSP_ERR_ARG, "op %d: bad BI_LEVEL_ZERO_CROSSING (dst, ip[0]: the slots of polarity_out and t_trig_times_out; ip[1]: the register of the count)", i);
            if (slot_len[o.dst] != slot_len[o.ip[0]])
                return fail(DSP_ERR_ARG, "bi_level_zero_crossing_time_points: the output arrays are of different lengths (%d and %d)", slot_len[o.dst], slot_len[o.ip[0]]);
            if (slot_len[o.dst] < 1) return fail(DSP_ERR_ARG, "bi_level_zero_crossing_time_points: polarity_out and t_trig_times_out hold at least one entry");
            if (o.sp[2].kind == DSP_ARG_CONST && !std::isfinite(o.sp[2].value))
                return fail(DSP_ERR_ARG, "bi_level_zero_crossing_time_points: gate_time_in is a finite number of samples");
            // t_start: the reference's checks in its order (time_point_thresh.py:479-483), for a constant
            if (o.sp[3].kind == DSP_ARG_CONST && !std::isnan(o.sp[3].value)) {
                const double t = op_const(c, o, 3);
                if (floor(t) != t) return fail(DSP_E_TPT_START_INT, "%s", dsp_fatal_message(DSP_E_TPT_START_INT));
                if (t < 0 || t >= slot_len[o.src]) return fail(DSP_E_TPT_RANGE, "%s", dsp_fatal_message(DSP_E_TPT_RANGE));
            }
            if (!f64 && slot_len[o.src] > (1 << 24))
                return fail(DSP_ERR_UNSUPPORTED, "bi_level_zero_crossing_time_points: the float32 loop takes rows of at most 2^24 samples (%d): a time counts them exactly", slot_len[o.src]);
            break;
        }
        case DSP_OP_PEAK_SNR_THRESHOLD: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || !check_slot(P, o.ip[0]) || o.dst == o.src || o.ip[0] == o.src || o.dst == o.ip[0] || o.ip[1] < 0 ||
                o.ip[1] >= n_sregs)
                return fail(DSP_ERR_ARG, "op %d: bad PEAK_SNR_THRESHOLD (src: the slot of the row; ip[0]: the slot of idx_in; dst: another slot, for idx_out; ip[1]: the register of the count)", i);
            if (slot_len[o.dst] != slot_len[o.ip[0]])
                return fail(DSP_ERR_ARG, "peak_snr_threshold: idx_out has the length of idx_in (%d and %d)", slot_len[o.dst], slot_len[o.ip[0]]);
            if (slot_len[o.dst] > DSP_PEAKS_MAX)
                return fail(DSP_ERR_UNSUPPORTED, "peak_snr_threshold: at most %d candidates (%d given): a wavefront keeps one per lane", DSP_PEAKS_MAX, slot_len[o.dst]);
            if (o.sp[1].kind != DSP_ARG_CONST)
                return fail(DSP_ERR_UNSUPPORTED, "peak_snr_threshold: width_in is a constant of the program, not a per-event value");
            if (!(o.sp[1].value >= 0) || !std::isfinite(o.sp[1].value)) return fail(DSP_ERR_ARG, "peak_snr_threshold: width_in is a non-negative number of samples");
            break;
        }
        case DSP_OP_MULTI_A_FILTER: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || !check_slot(P, o.ip[0]) || o.dst == o.src || o.ip[0] == o.src || o.dst == o.ip[0])
                return fail(DSP_ERR_ARG, "op %d: bad MULTI_A_FILTER (src: the slot of the row; ip[0]: the slot of vt_maxs_in; dst: another slot, for va_max_out)", i);
            if (slot_len[o.dst] != slot_len[o.ip[0]])
                return fail(DSP_ERR_ARG, "multi_a_filter: va_max_out has the length of vt_maxs_in (%d and %d)", slot_len[o.dst], slot_len[o.ip[0]]);
            if (slot_len[o.dst] > DSP_PEAKS_MAX)
                return fail(DSP_ERR_UNSUPPORTED, "multi_a_filter: at most %d positions (%d given): a wavefront keeps one per lane", DSP_PEAKS_MAX, slot_len[o.dst]);
            if (!(slot_len[o.ip[0]] < slot_len[o.src])) return fail(DSP_E_MAF_LEN, "%s", dsp_fatal_message(DSP_E_MAF_LEN));  // multi_a_filter.py:42-45
            break;
        }
        case DSP_OP_LOG_CHECK: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || o.dst == o.src)
                return fail(DSP_ERR_ARG, "op %d: bad LOG_CHECK (src: the slot of the row; dst: another slot, for the logged row)", i);
            if (slot_len[o.dst] != slot_len[o.src])
                return fail(DSP_ERR_ARG, "log_check: the output has the length of the input (len(w_in) = %d, len(w_log) = %d)", slot_len[o.src], slot_len[o.dst]);
            break;
        }
        case DSP_OP_POLY_FIT: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || o.dst == o.src)
                return fail(DSP_ERR_ARG, "op %d: bad POLY_FIT (src: the slot of the row; dst: another slot, for the coefficients; io: the inverted matrix)", i);
            const int m = slot_len[o.dst];
            if (m > DSP_POLY_MAX) return fail(DSP_ERR_UNSUPPORTED, "poly_fit: " DSP_POLY_MAX_TEXT, DSP_POLY_MAX, m);
            if (!need_io(c, o, DSP_IO_TAPS) || c.io[o.io].dtype != DSP_F64 || c.io[o.io].len != m * m)
                return fail(DSP_ERR_ARG, "poly_fit: io is a DSP_IO_TAPS binding of m * m = %d DSP_F64 values, the inverted matrix of power sums (both loops)", m * m);
            if (!dsp_poly_powers_fit(slot_len[o.src], m)) return fail(DSP_ERR_UNSUPPORTED, "poly_fit: " DSP_POLY_POWER_TEXT, slot_len[o.src], m);
            break;
        }
        case DSP_OP_POLY_DIFF:
        case DSP_OP_POLY_EXP_RMS: {
            const char* name = o.opcode == DSP_OP_POLY_DIFF ? "poly_diff" : "poly_exp_rms";
            if (!check_slot(P, o.src) || !check_slot(P, o.ip[0]) || o.ip[0] == o.src || o.dst < 0 || o.dst + 1 >= n_sregs)
                return fail(DSP_ERR_ARG, "op %d: bad %s (src: the slot of the row; ip[0]: the slot of the coefficients; dst, dst + 1: the registers of mean and rms)", i,
                            o.opcode == DSP_OP_POLY_DIFF ? "POLY_DIFF" : "POLY_EXP_RMS");
            const int m = slot_len[o.ip[0]];
            if (m > DSP_POLY_MAX) return fail(DSP_ERR_UNSUPPORTED, "%s: " DSP_POLY_MAX_TEXT, name, DSP_POLY_MAX, m);
            if (!dsp_poly_powers_fit(slot_len[o.src], m)) return fail(DSP_ERR_UNSUPPORTED, "%s: " DSP_POLY_POWER_TEXT, name, slot_len[o.src], m);
            break;
        }
        case DSP_OP_INL_CORRECTION: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || o.dst == o.src)
                return fail(DSP_ERR_ARG, "op %d: bad INL_CORRECTION (src: the slot of the row; dst: another slot, for the corrected row; io: the table)", i);
            if (slot_len[o.dst] != slot_len[o.src])
                return fail(DSP_ERR_ARG, "inl_correction: the output has the length of the input (len(w_in) = %d, len(w_out) = %d)", slot_len[o.src], slot_len[o.dst]);
            if (!need_io(c, o, DSP_IO_TAPS) || c.io[o.io].dtype != c.compute_dtype || c.io[o.io].len < 1)
                return fail(DSP_ERR_ARG, "inl_correction: io is a DSP_IO_TAPS binding of the p >= 1 entries of inl in the loop's type");
            break;
        }
        case DSP_OP_WF_CENTROID: {
            if (!check_slot(P, o.src) || o.dst < 0 || o.dst >= n_sregs)
                return fail(DSP_ERR_ARG, "op %d: bad WF_CENTROID (src: the slot of the row; dst: the register of the centroid)", i);
            if (o.sp[0].kind != DSP_ARG_CONST) return fail(DSP_ERR_UNSUPPORTED, "get_wf_centroid: shift is a constant of the program, not a per-event value");
            const double shift = op_const(c, o, 0);  // get_wf_centroid.py:55-60
            if (std::isnan(shift)) return fail(DSP_ERR_ARG, "shift is nan");
            if (shift < 0) return fail(DSP_ERR_ARG, "shift must be positive");
            if (shift > slot_len[o.src] - 1) return fail(DSP_ERR_ARG, "shift must be shorter than input waveform size");
            break;
        }
        case DSP_OP_WF_ALIGNMENT: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || o.dst == o.src)
                return fail(DSP_ERR_ARG, "op %d: bad WF_ALIGNMENT (src: the slot of the row; dst: another slot, for the window; sp: centroid, shift, size)", i);
            if (o.sp[0].kind == DSP_ARG_REG) return fail(DSP_ERR_UNSUPPORTED, "wf_alignment: centroid is a constant or a per-event column, not a register of the program");
            if (o.sp[1].kind != DSP_ARG_CONST) return fail(DSP_ERR_UNSUPPORTED, "wf_alignment: shift is a constant of the program, not a per-event value");
            if (o.sp[2].kind != DSP_ARG_CONST) return fail(DSP_ERR_UNSUPPORTED, "wf_alignment: size is a constant of the program, not a per-event value");
            const int n = slot_len[o.src];
            const double shift = op_const(c, o, 1), size = op_const(c, o, 2);  // wf_alignment.py:63-78
            if (o.sp[0].kind == DSP_ARG_CONST && std::isnan(o.sp[0].value)) return fail(DSP_E_ALIGN_CENTROID, "%s", dsp_fatal_message(DSP_E_ALIGN_CENTROID));
            if (std::isnan(shift)) return fail(DSP_ERR_ARG, "shift is nan");
            if (shift < 0) return fail(DSP_ERR_ARG, "shift must be positive");
            if (shift > n) return fail(DSP_ERR_ARG, "shift must be shorter than input waveform size");
            if (std::isnan(size)) return fail(DSP_ERR_ARG, "size is nan");
            if (size <= 0) return fail(DSP_ERR_ARG, "size must be positive");
            if (size > n) return fail(DSP_ERR_ARG, "size must be shorter than input waveform size");
            if (size != (double)slot_len[o.dst])
                return fail(DSP_ERR_ARG, "wf_alignment: size is a whole number and equals len(w_out) (size = %g, len(w_out) = %d)", size, slot_len[o.dst]);
            break;
        }
        case DSP_OP_WF_CORRECTION: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || o.dst == o.src)
                return fail(DSP_ERR_ARG, "op %d: bad WF_CORRECTION (src: the slot of the row; dst: another slot, for the corrected row; io: w_corr; ip: start_idx, stop_idx)", i);
            if (slot_len[o.dst] != slot_len[o.src])
                return fail(DSP_ERR_ARG, "wf_correction: the output has the length of the input (len(w_in) = %d, len(w_out) = %d)", slot_len[o.src], slot_len[o.dst]);
            if (!need_io(c, o, DSP_IO_TAPS) || c.io[o.io].dtype != c.compute_dtype)
                return fail(DSP_ERR_ARG, "wf_correction: io is a DSP_IO_TAPS binding of w_corr in the loop's type");
            const int n = slot_len[o.src], start = o.ip[0], stop = o.ip[1];  // wf_correction.py:64-77
            if (start < 0) return fail(DSP_ERR_ARG, "start_idx must be positive");
            if (start > n) return fail(DSP_ERR_ARG, "start_idx must be shorter than input waveform size");
            if (stop <= 0) return fail(DSP_ERR_ARG, "stop_idx must be positive");
            if (stop > n) return fail(DSP_ERR_ARG, "stop_idx must be shorter than input waveform size");
            if (start >= stop) return fail(DSP_ERR_ARG, "start_idx must be smaller than stop_idx");
            if (stop - start > c.io[o.io].len) return fail(DSP_ERR_ARG, "stop_idx - start_idx must be smaller than len(w_corr)");
            break;
        }
        case DSP_OP_DWT_HAAR: {
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || !check_slot(P, o.ip[2]) || o.dst == o.src || o.dst == o.ip[2])
                return fail(DSP_ERR_ARG, "op %d: bad DWT_HAAR slots", i);
            if (o.ip[0] <= 0) return fail(DSP_E_DWT_LEVEL, "%s", dsp_fatal_message(DSP_E_DWT_LEVEL));
            if (o.ip[1] != 'a' && o.ip[1] != 'd') return fail(DSP_ERR_ARG, "op %d: DWT coefficient must be 'a' or 'd'", i);
            int len = slot_len[o.src];
            if (slot_len[o.ip[2]] < (len + 1) / 2 && o.ip[0] > 1) return fail(DSP_ERR_ARG, "op %d: DWT scratch slot too small", i);
            for (int l = 0; l < o.ip[0]; ++l) len = (len + 1) / 2;
            if (len != slot_len[o.dst]) return fail(DSP_E_DWT_OUTLEN, "%s (got %d, expect %d)", dsp_fatal_message(DSP_E_DWT_OUTLEN), slot_len[o.dst], len);
            break;
        }
        case DSP_OP_COPY: {  // dst[k] = src[ip[0] + k * step], step = ip[1] (0 means 1; negative: backwards)
            const int64_t step = o.ip[1] != 0 ? o.ip[1] : 1;
            const int64_t last = check_slot(P, o.dst) ? (int64_t)o.ip[0] + (int64_t)(slot_len[o.dst] - 1) * step : -1;
            if (!check_slot(P, o.src) || !check_slot(P, o.dst) || o.src == o.dst || o.ip[0] < 0 || o.ip[0] >= slot_len[o.src] || last < 0 ||
                last >= slot_len[o.src])
                return fail(DSP_ERR_ARG, "op %d: bad COPY", i);
            break;
        }
        case DSP_OP_ELEMENTWISE: {
            if (!check_slot(P, o.dst) || !fn_code_ok(o.ip[0], f64)) return fail(DSP_ERR_ARG, "op %d: bad ELEMENTWISE", i);
            const int opnd[3] = {o.src, o.ip[1], o.ip[2]};
            int n_wf_opnd = 0;
            for (int k = 0; k < 3; ++k) {
                if (opnd[k] < 0) continue;
                if (!check_slot(P, opnd[k]) || slot_len[opnd[k]] != slot_len[o.dst])
                    return fail(DSP_ERR_ARG, "op %d: ELEMENTWISE operand %d is not a waveform of the length of the result", i, k);
                ++n_wf_opnd;
            }
            if (!n_wf_opnd) return fail(DSP_ERR_ARG, "op %d: ELEMENTWISE needs a waveform operand (DSP_OP_SCALAR_FUNC otherwise)", i);
            break;
        }
        case DSP_OP_SCALAR_FUNC:
            if (o.dst < 0 || o.dst >= n_sregs || !fn_code_ok(o.ip[0], f64, i64)) return fail(DSP_ERR_ARG, "op %d: bad SCALAR_FUNC", i);
            break;
        case DSP_OP_CONVOLVE:
        case DSP_OP_CONVOLVE_AMAX: return lower_convolve(c, i, o, d);
        case DSP_OP_SCALAR_AFFINE:
        case DSP_OP_SCALAR_DIV:
            if (o.dst < 0 || o.dst >= n_sregs) return fail(DSP_ERR_ARG, "op %d: bad scalar arithmetic op", i);
            break;
        case DSP_OP_SCALAR_CONVERT:
            if (o.dst < 0 || o.dst >= n_sregs || o.ip[0] < 0 || o.ip[0] > 4 || o.sp[3].kind != DSP_ARG_CONST)
                return fail(DSP_ERR_ARG, "op %d: bad SCALAR_CONVERT (ip[0] = rounding 0..4, sp[3] = constant period ratio)", i);
            break;
        default: return fail(DSP_ERR_ARG, "op %d: unknown opcode %d", i, o.opcode);
    }
    return DSP_OK;
}

// ---- ops: the device program, an op of the caller's after the other, each behind the clearing ops of the shared slots it is the first to use
static int lower_ops(PlanCtx& c) {
    DevProgram& P = c.ch->host;
    c.dev_index.assign(c.n_ops, 0);
    for (int i = 0; i < c.n_ops; ++i) {
        const dsp_op& o = c.ops[i];
        for (int s = 0; s < c.n_slots; ++s)
            if (c.shares[s] && c.first_op[s] == i) {
                DevOp& z = P.ops[c.n_dev_ops++];
                memset(&z, 0, sizeof z);
                z.opcode = DSP_OP_INTERNAL_ZERO;
                z.dst = s;
                z.ic[0] = c.base[s];
                z.ic[1] = c.foot[s];
            }
        c.dev_index[i] = c.n_dev_ops;
        DevOp& d = P.ops[c.n_dev_ops++];
        memset(&d, 0, sizeof d);
        d.opcode = o.opcode;
        d.dst = o.dst;
        d.src = o.src;
        d.io = o.io;
        memcpy(d.ip, o.ip, sizeof d.ip);
        memcpy(d.sp, o.sp, sizeof d.sp);
        for (int k = 0; k < 4; ++k) {
            const dsp_scalar_arg& a = o.sp[k];
            if (a.kind == DSP_ARG_INPUT && (a.index < 0 || a.index >= c.n_io || c.io[a.index].kind != DSP_IO_SCALAR_IN))
                return fail(DSP_ERR_ARG, "op %d: scalar operand %d is not a scalar input binding", i, k);
            if (a.kind == DSP_ARG_REG && (a.index < 0 || a.index >= c.n_sregs)) return fail(DSP_ERR_ARG, "op %d: bad scalar register", i);
            if (a.kind < DSP_ARG_CONST || a.kind > DSP_ARG_REG) return fail(DSP_ERR_ARG, "op %d: bad scalar operand kind", i);
        }
        if (const int rc = lower_op(c, i, o, d)) return rc;
    }
    P.n_ops = c.n_dev_ops;
    return DSP_OK;
}

// LOAD s; BL_SUBTRACT s <- s (what nearly every recipe starts with): the load subtracts while it writes the samples to LDS and the
// second op becomes a no-op -- one pass over the waveform in LDS less.  Same results: one float subtraction per sample in the loop's
// type, and the NaN rule of bl_subtract.py:41-44 (a NaN anywhere, or a NaN baseline: a NaN waveform) is the load's own flag.
static void fold_load_bl_subtract(PlanCtx& c) {
    DevProgram& P = c.ch->host;
    const std::vector<int>& dev_index = c.dev_index;
    for (int i = 0; i + 1 < c.n_ops; ++i) {
        const dsp_op &ld = c.ops[i], &bs = c.ops[i + 1];
        if (ld.opcode == DSP_OP_LOAD && bs.opcode == DSP_OP_BL_SUBTRACT && bs.src == ld.dst && bs.dst == ld.dst && bs.ip[0] == 0 &&
            dev_index[i + 1] == dev_index[i] + 1) {
            DevOp& L = P.ops[dev_index[i]];
            DevOp& B = P.ops[dev_index[i + 1]];
            L.ic[0] = 1;
            L.sp[0] = B.sp[0];
            B.opcode = DSP_OP_INTERNAL_NOP;
        }
    }
}

// Carry plan of the register-resident energy kernel (EnergyPlan, dsp_plan.h): Ci samples per lane, S replay sub-chains of (Ci - 2) / S
// samples (the chunk's last two extend the last one), the three lags of the trapezoid.  Sub-chain s of a lane starts at sample s CS of its
// chunk; its lagged stream k starts `lag` samples lower, r samples into the chunk of the lane `shift` below (0 <= r < Ci).  The carry is
// the prefix sum of those r samples: the side array's group-end sum in front of the 8-sample group that holds sample r - 1 (none in
// front of group 0) plus the first pn samples of that group -- all of it in the form the kernel uses without arithmetic of its own.
extern "C" void dsp_internal_plan_energy_carries(int Ci, int S, const int32_t* lags, EnergyPlan* plan) {
    const int CS = (Ci - 2) / S;
    for (int k = 0; k < 3; ++k)
        for (int sidx = 0; sidx < 4; ++sidx) {
            const bool used = sidx < S;
            const int pos = used ? sidx * CS - lags[k] : 0;  // samples before the sub-chain start, relative to the chunk
            const int r = ((pos % Ci) + Ci) % Ci;             // ... = r samples into the chunk of the lane `shift` below
            const int gi = (r > 0 ? r - 1 : 0) >> 3;          // group that holds sample r - 1 (group (Ci - 2) / 8: the two-sample tail)
            const int cs = r / CS > S - 1 ? S - 1 : r / CS;
            plan->shift[k][sidx] = (r - pos) / Ci;
            plan->cs[k][sidx] = cs;
            plan->local[k][sidx] = r - cs * CS;
            plan->grp[k][sidx] = 8 * gi;
            plan->side[k][sidx] = gi - 1;  // (-1: nothing in front)
            plan->pn[k][sidx] = r - 8 * gi;
        }
}

// Register-resident kernel: C = len/64 + 2 samples per lane (an even pitch: every lane's chunk is 8-byte aligned), linear LDS
// image of the waveform (1024 .. 8192 samples); a chunk is (C - 2) / 8 groups of 8 samples and a two-sample tail
static void plan_energy_rr(PlanCtx& c, const DevOp& dtp) {
    ChainPlan* ch = c.ch;
    EnergyArgs& I = ch->rr;
    I = ch->fused;
    const int Ci = c.slot_len[0] / 64 + 2;
    I.C = Ci;
    I.pitch = Ci;
    I.invC = 1.0f / (float)Ci;
    const dsp_energy_rr::Layout L = dsp_energy_rr::layout(Ci);  // (the kernel addresses the region by the same)
    I.slot_off = L.slot_off;
    I.lds_elems_per_wave = L.elems;
    ch->rr_lds_bytes = L.elems * 4;
    for (int k = 0; k < 3; ++k) {
        I.q[k] = dtp.ic[k];  // the lags themselves
        I.rho[k] = 0;
    }
    for (int S = 1; S <= 2; ++S) dsp_internal_plan_energy_carries(Ci, S, dtp.ic, &ch->plan[S - 1]);
    ch->rr_ok = true;
    ch->variant = 6;
    if (const char* venv = getenv("DSPEED_HIP_VARIANT")) ch->variant = atoi(venv);  // A/B runs: 1, 6, 8
    if (ch->variant != 1 && ch->variant != 8) ch->variant = 6;
}

// ---- does the program have the shape LOAD [-> BL_SUBTRACT] -> POLE_ZERO -> TRAP_PICKOFF -> STORE_SCALAR on one slot?
static void match_energy_shape(PlanCtx& c) {
    ChainPlan* ch = c.ch;
    const DevProgram& P = ch->host;
    const dsp_op* ops = c.ops;
    const dsp_io_desc* io = c.io;
    const int32_t* slot_len = c.slot_len;
    const int n_ops = c.n_ops, n_slots = c.n_slots;
    const bool f64 = c.f64;
    int i = 0;
    const dsp_op* ld = (n_ops > i && ops[i].opcode == DSP_OP_LOAD) ? &ops[i++] : nullptr;
    const dsp_op* bs = (ld && n_ops > i && ops[i].opcode == DSP_OP_BL_SUBTRACT) ? &ops[i++] : nullptr;
    const dsp_op* pz = (ld && n_ops > i && ops[i].opcode == DSP_OP_POLE_ZERO) ? &ops[i++] : nullptr;
    const dsp_op* tp = (pz && n_ops > i && ops[i].opcode == DSP_OP_TRAP_PICKOFF) ? &ops[i++] : nullptr;
    const dsp_op* st = (tp && n_ops > i && ops[i].opcode == DSP_OP_STORE_SCALAR) ? &ops[i++] : nullptr;
    const int wdt = ld ? io[ld->io].dtype : -1;
    // (a time constant per event, a float32 column: the register-resident kernel's TAU builds form exp(-1/tau) per row like the interpreter's op)
    const bool tau_col = pz && pz->sp[0].kind == DSP_ARG_INPUT && io[pz->sp[0].index].dtype == DSP_F32;
    const bool shape = !f64 && st && i == n_ops && n_slots == 1 && ld->ip[0] == 0 && ld->ip[1] == 0 && (wdt == DSP_F32 || wdt == DSP_I16 || wdt == DSP_U16) && P.io[ld->io].vec_ok &&
                       (!bs || (bs->dst == 0 && bs->src == 0 && bs->sp[0].kind != DSP_ARG_REG)) && pz->dst == 0 && pz->src == 0 &&
                       (pz->sp[0].kind == DSP_ARG_CONST || tau_col) &&
                       tp->src == 0 && tp->sp[0].kind != DSP_ARG_REG && st->ip[0] == tp->dst &&
                       (slot_len[0] == 1024 || slot_len[0] == 2048 || slot_len[0] == 4096 || slot_len[0] == 8192);
    if (!shape && st && i == n_ops && n_slots == 1) {  // the ops of the energy chain, but not the kernels' case of it
        if (f64) note(ch, "the energy chain in a float64 loop: the fused energy kernels are float32");
        else if (pz->sp[0].kind != DSP_ARG_CONST && !tau_col)
            note(ch, "a pole-zero time constant per event that is not a float32 column: the fused energy kernels take a constant or such a column");
        else if (!(slot_len[0] == 1024 || slot_len[0] == 2048 || slot_len[0] == 4096 || slot_len[0] == 8192))
            note(ch, "waveforms of %d samples: the fused energy kernels take 1024, 2048, 4096 or 8192", slot_len[0]);
        else if (!P.io[ld->io].vec_ok) note(ch, "rows that do not start on 16-byte boundaries: the fused energy kernels read 16 bytes per lane");
    }
    auto f32_col = [&](const dsp_scalar_arg& a) { return a.kind != DSP_ARG_INPUT || io[a.index].dtype == DSP_F32; };
    if (shape && (!bs || f32_col(bs->sp[0])) && f32_col(tp->sp[0]) && io[st->io].dtype == DSP_F32) {  // (the kernels store a float)
        EnergyArgs& F = ch->fused;
        const DevOp& dpz = P.ops[c.dev_index[pz - ops]];
        const DevOp& dtp = P.ops[c.dev_index[tp - ops]];
        F.wf_stride = io[ld->io].row_stride;
        F.wf_offset = io[ld->io].offset;
        F.len = slot_len[0];
        F.has_bl = bs ? 1 : 0;
        if (bs) {
            if (bs->sp[0].kind == DSP_ARG_INPUT) {
                ch->io_bl = bs->sp[0].index;
                F.bl_stride = io[ch->io_bl].row_stride;
            } else {
                F.bl_const = (float)bs->sp[0].value;
            }
        }
        if (tp->sp[0].kind == DSP_ARG_INPUT) {
            ch->io_tp = tp->sp[0].index;
            F.tp_stride = io[ch->io_tp].row_stride;
        } else {
            F.tp_const = (float)tp->sp[0].value;
        }
        F.mode = tp->io;
        F.out_stride = io[st->io].row_stride;
        F.c = dpz.fc[0];
        F.tau_nan = dpz.ic[0];
        F.rr = dtp.fc[0];
        F.ll = dtp.fc[1];
        F.all_nan = dtp.ic[9];
        F.C = P.slots[0].C;
        F.pitch = P.slots[0].pitch;
        F.invC = P.slots[0].invC;
        for (int k = 0; k < 3; ++k) {
            F.q[k] = dtp.ic[3 + k];
            F.rho[k] = dtp.ic[6 + k];
        }
        F.lds_elems_per_wave = P.lds_elems_per_wave;
        F.slot_off = P.slots[0].off;
#ifdef DSPEED_HIP_DIAG
        if (const char* ab = getenv("DSPEED_HIP_ABLATE")) F.ablate = atoi(ab);  // diagnostic library only: skip passes / stamp phases
#endif
        ch->io_wf = ld->io;
        ch->io_out = st->io;
        ch->fused_trap = tp->ip[3];
        ch->fused_npf = slot_len[0] / 256;          // one wavefront per waveform: len == 256 * npf, npf in {4, 8, 16}
        ch->fused_ok = slot_len[0] <= 4096 && wdt == DSP_F32 && !tau_col;  // the classic kernel reads float32 rows only, one time constant
        if (tau_col) {
            ch->io_tau = pz->sp[0].index;
            F.tau_stride = io[ch->io_tau].row_stride;
        }
        ch->wf_dtype = wdt;
        plan_energy_rr(c, dtp);
    }
}

// the amax form runs on the float16 matrix instructions (two-way split operands, float32-accurate: dsp_fir_f16.hip) unless asked
// for the float32 ones (DSPEED_HIP_FIR_F32=1: A/B and the exact float32 chain); its staging loads are 16 bytes of any row type
static void choose_fir_f16(PlanCtx& c) {
    ChainPlan* ch = c.ch;
    const char* f32 = getenv("DSPEED_HIP_FIR_F32");
    const dsp_io_desc& w = c.io[ch->fio_wf];
    const int es = w.dtype == DSP_F32 ? 4 : 2;
    const int n_slice = ch->fir.n;  // (its 8-sample vectors are read whole: the last one must end inside the row)
    if (!(f32 && f32[0] == '1') && (w.row_stride * es) % 16 == 0 && (w.offset * es) % 16 == 0 &&
        ((n_slice & 7) == 0 || w.offset + ((n_slice + 7) & ~7) <= w.row_stride)) {
        ch->fir_f16 = true;
        ch->f16.tz = dsp_fir_f16::tz(ch->fir.kend);
    }
}

// nothing but arithmetic between per-event values and stores: one row per lane instead of one per wavefront
static bool match_scalar_shape(const PlanCtx& c) {
    bool only_scalar = true;
    for (int i = 0; i < c.n_ops; ++i) {
        const int oc = c.ops[i].opcode;
        only_scalar &= oc == DSP_OP_SCALAR_AFFINE || oc == DSP_OP_SCALAR_DIV || oc == DSP_OP_SCALAR_CONVERT || oc == DSP_OP_SCALAR_FUNC ||
                       oc == DSP_OP_STORE_SCALAR;
    }
    return only_scalar && c.n_dev_ops == c.n_ops;
}

uint64_t dsp_plan_switches() {
    static const char* const names[] = {"DSPEED_HIP_VARIANT", "DSPEED_HIP_ABLATE", "DSPEED_HIP_FIR_F32", "DSPEED_HIP_NO_FUSED", "DSPEED_HIP_NO_FIR_RUNS",
                                        "DSPEED_HIP_NO_THRESHOLD_FOLD", "DSPEED_HIP_NO_TEAMS", "DSPEED_HIP_TEAM_MAX", "DSPEED_HIP_TEAM_WPB"};
    uint64_t h = 1469598103934665603ull;  // (FNV-1a over the values, a separator behind each)
    for (const char* name : names) {
        const char* v = getenv(name);
        for (const char* p = v ? v : ""; *p; ++p) h = (h ^ (unsigned char)*p) * 1099511628211ull;
        h = (h ^ 0xffu) * 1099511628211ull;
    }
    return h;
}

// Every specialised kernel's shape against the program: the *_ok flags, the kernels' argument blocks and binding indices.  Several may
// hold at once; which kernel runs is dsp_plan_route's business (and, with the pointers of a launch in hand, dsp_chain_execute's).
static void match_shapes(PlanCtx& c) {
    ChainPlan* ch = c.ch;
    const char* env = getenv("DSPEED_HIP_NO_FUSED");  // every specialised kernel off: the interpreter runs the program
    ch->fused_on = !(env && env[0] == '1');
    match_energy_shape(c);
    ch->fir_ok = match_fir_shape(c);
    if (!ch->fir_ok) {
        for (int k = 0; k < DSP_FIR_MAXK; ++k) ch->fio_taps[k] = ch->fio_out[k] = -1;
        ch->fir_ok = match_fir_store_shape(c);
    }
    if (ch->fir_ok) choose_fir_f16(c);
    ch->rows_ok = match_rows_shape(c);
    if (!ch->rows_ok) {
        ch->rio_wf = ch->rio_bl = ch->rio_thr = ch->rio_ts = ch->rio_tpt = ch->rio_dwt = -1;
        for (int k = 0; k < 4; ++k) ch->rio_mm[k] = -1;
    }
    ch->scalar_ok = match_scalar_shape(c);
    ch->pz_ok = match_pz_rows_shape(c);
    ch->red_ok = match_reduce_shape(c);
    const char* off = getenv("DSPEED_HIP_NO_FIR_RUNS");  // A/B runs: the matrix-core FIR for piecewise-constant kernels too
    if (!ch->red_ok && !(off && off[0] == '1')) ch->runs_ok = match_fir_runs_shape(c);
    if (ch->runs_ok) ch->fir_ok = ch->fir_f16 = false;  // (LOAD, CONVOLVE, STORE has the matrix-core kernel's shape as well)
    ch->cur_ok = match_current_shape(c);
    if (!ch->cur_ok) {
        ch->cio_wf = ch->cio_t0 = -1;
        for (int k = 0; k < 4; ++k) ch->cio_out[k] = -1;
    }
}

// scalar registers an op writes (waveform ops name a slot in dst: to the threshold fold a spurious match only ends a window early, and
// a program that forms teams holds none behind its load)
static int written_regs(const DevOp& o, int* r) {
    int n = 0;
    switch (o.opcode) {
        case DSP_OP_MIN_MAX: for (int k = 0; k < 4; ++k) r[n++] = o.dst + k; break;
        case DSP_OP_TRAP_REDUCE:
            if (o.dst >= 0) for (int k = 0; k < 4; ++k) r[n++] = o.dst + k;
            if (o.io >= 0) r[n++] = o.io;
            if ((((o.ip[3] >> 16) & 0x3fff) - 1) >= 0) r[n++] = ((o.ip[3] >> 16) & 0x3fff) - 1;  // (a pick-off that reads the same trapezoid)
            break;
        case DSP_OP_LOAD: case DSP_OP_STORE: case DSP_OP_STORE_SCALAR: case DSP_OP_INTERNAL_NOP: case DSP_OP_INTERNAL_ZERO: break;
        default: r[n++] = o.dst;
    }
    return n;
}
static bool writes_reg(const DevOp& o, int r) {
    int w[8];
    const int n = written_regs(o, w);
    return std::find(w, w + n, r) != w + n;
}

// ---- a threshold that is a fraction of a per-event value (the rise-time walks of the Ge recipes: time_point_thresh at 0.99 / 0.9 / 0.5 /
// 0.1 of the trapezoid's maximum) costs the interpreter an op of its own -- ~ 1 700 cycles of a row's lone wavefront, whatever the op
// computes -- for one multiplication.  SCALAR_AFFINE d <- x * const + 0 whose result only TIME_POINT_THRESH ops read as their threshold
// is folded into them: they multiply (the same float multiplication: x * b + (+-0) is x * b) and the op becomes a no-op.
static void fold_scaled_thresholds(PlanCtx& c) {
    DevProgram& P = c.ch->host;
    const char* nf = getenv("DSPEED_HIP_NO_THRESHOLD_FOLD");  // (A/B runs and the bit-identity test)
    if (nf && nf[0] == '1') return;
    for (int i = 0; i < P.n_ops; ++i) {
        DevOp& a = P.ops[i];
        if (a.opcode != DSP_OP_SCALAR_AFFINE || a.sp[0].kind != DSP_ARG_REG || a.sp[1].kind != DSP_ARG_CONST || a.sp[2].kind != DSP_ARG_CONST ||
            a.sp[2].value != 0.0 || a.sp[0].index == a.dst)
            continue;
        const int r = a.dst, x = a.sp[0].index;
        std::vector<int> users;
        bool fine = true;
        for (int j = i + 1; j < P.n_ops && fine; ++j) {
            const DevOp& o = P.ops[j];
            bool reads_r = false;
            for (int k = 0; k < 4; ++k)
                if (o.sp[k].kind == DSP_ARG_REG && o.sp[k].index == r) {
                    reads_r = true;
                    if (!(o.opcode == DSP_OP_TIME_POINT_THRESH && k == 0 && o.ic[0] == 0)) fine = false;
                }
            if (o.opcode == DSP_OP_STORE_SCALAR && o.ip[0] == r) fine = false;
            if (reads_r && fine) users.push_back(j);
            if (writes_reg(o, r)) break;                        // the register starts another life: what follows reads that
            if (writes_reg(o, x) && fine) {                     // the value the walks would multiply changes here: nothing may read r after it
                for (int j2 = j + 1; j2 < P.n_ops; ++j2) {
                    const DevOp& o2 = P.ops[j2];
                    for (int k = 0; k < 4; ++k)
                        if (o2.sp[k].kind == DSP_ARG_REG && o2.sp[k].index == r) fine = false;
                    if (o2.opcode == DSP_OP_STORE_SCALAR && o2.ip[0] == r) fine = false;
                    if (writes_reg(o2, r)) break;
                }
                break;
            }
        }
        if (!fine || users.empty()) continue;
        for (int j : users) {
            P.ops[j].sp[0] = a.sp[0];
            P.ops[j].ic[0] = 1;
            P.ops[j].fc[0] = a.sp[1].value;
        }
        a.opcode = DSP_OP_INTERNAL_NOP;
    }
}

// ---- a team of two wavefronts per row?  A program that loads ONE waveform and then only reads it -- the trapezoid reductions, pick-offs and
// walks a whole recipe runs on its pole-zero rows -- whose image leaves LDS for one wavefront per SIMD: its ops fall into groups that share
// no scalar register, and two wavefronts can run two groups on the one image at the same time.
static void form_teams(PlanCtx& c) {
    ChainPlan* ch = c.ch;
    DevProgram& P = ch->host;
    P.team = 1;
    for (int i = 0; i < P.n_ops; ++i) P.ops[i].member = DSP_MEMBER_ALL;
    const char* env = getenv("DSPEED_HIP_NO_TEAMS");
    const bool vm_runs = !(ch->fused_ok || ch->rr_ok || ch->rows_ok || ch->fir_ok || ch->cur_ok || ch->red_ok || ch->pz_ok || ch->scalar_ok);
    bool ok = vm_runs && !(env && env[0] == '1') && !c.f64 && !ch->has_fir && c.n_slots == 1 && ch->lds_bytes_per_wave > 0 &&
              LDS_BYTES_PER_CU / ch->lds_bytes_per_wave <= 4 && ch->waves_per_block * 2 <= 16 && c.n_sregs <= 128;
    int first = 0;
    while (first < P.n_ops && P.ops[first].opcode == DSP_OP_INTERNAL_NOP) ++first;
    ok = ok && first < P.n_ops && P.ops[first].opcode == DSP_OP_LOAD;
    for (int i = first + 1; ok && i < P.n_ops; ++i) {
        switch (P.ops[i].opcode) {
            case DSP_OP_TRAP_REDUCE: case DSP_OP_TRAP_PICKOFF: case DSP_OP_TIME_POINT_THRESH: case DSP_OP_PICKOFF: case DSP_OP_MIN_MAX: case DSP_OP_AMAX:
            case DSP_OP_SCALAR_AFFINE: case DSP_OP_SCALAR_DIV: case DSP_OP_SCALAR_CONVERT: case DSP_OP_SCALAR_FUNC: case DSP_OP_STORE_SCALAR:
            case DSP_OP_INTERNAL_NOP: break;
            default: ok = false;
        }
    }
    if (!ok) return;
    // registers an op reads (scalar registers only: after the load nothing writes the waveform)
    auto reads = [&](const DevOp& o, int* r) {
        int n = 0;
        for (int k = 0; k < 4; ++k)
            if (o.sp[k].kind == DSP_ARG_REG) r[n++] = o.sp[k].index;
        if (o.opcode == DSP_OP_STORE_SCALAR) r[n++] = o.ip[0];
        return n;
    };
    // groups: ops joined by any register one writes and the other reads or writes
    std::vector<int> parent(P.n_ops);
    for (int i = 0; i < P.n_ops; ++i) parent[i] = i;
    auto find = [&](int x) { while (parent[x] != x) x = parent[x] = parent[parent[x]]; return x; };
    std::vector<int> owner(DSP_MAX_SREGS + 8, -1);  // register -> an op that touched it
    for (int i = first + 1; i < P.n_ops; ++i) {
        int regs[16], n = written_regs(P.ops[i], regs);
        n += reads(P.ops[i], regs + n);
        for (int k = 0; k < n; ++k) {
            const int r = regs[k];
            if (r < 0 || r >= (int)owner.size()) { ok = false; break; }
            if (owner[r] < 0) owner[r] = i;
            else parent[find(i)] = find(owner[r]);
        }
    }
    auto weight = [&](int oc) {
        switch (oc) {
            case DSP_OP_TRAP_REDUCE: return 27;
            case DSP_OP_TRAP_PICKOFF: return 20;
            case DSP_OP_MIN_MAX: return 16;
            case DSP_OP_TIME_POINT_THRESH: case DSP_OP_AMAX: return 4;
            case DSP_OP_PICKOFF: return 3;
            case DSP_OP_STORE_SCALAR: return 1;
            default: return 2;
        }
    };
    std::vector<int> w(P.n_ops, 0);
    for (int i = first + 1; i < P.n_ops; ++i) w[find(i)] += weight(P.ops[i].opcode);
    std::vector<int> roots;
    for (int i = first + 1; i < P.n_ops; ++i)
        if (find(i) == i) roots.push_back(i);
    std::sort(roots.begin(), roots.end(), [&](int a, int b) { return w[a] > w[b]; });
    // groups dealt out to two or three members, heaviest first, each to the member with the least so far (three: when the third
    // member still gets a real share -- the Ge recipe's program is a trapezoid with its five walks, a trapezoid with a pick-off and
    // a pick-off of a third: the recurrences are latency-bound, a third wavefront on the image fills a SIMD's idle issue slots)
    int load[3] = {0, 0, 0}, n_team = 2;
    std::vector<int> side(P.n_ops, 0);
    auto deal = [&](int members) {
        load[0] = load[1] = load[2] = 0;
        for (int r : roots) {
            int m = 0;
            for (int k = 1; k < members; ++k)
                if (load[k] < load[m]) m = k;
            side[r] = m;
            load[m] += w[r];
        }
    };
    const char* t3 = getenv("DSPEED_HIP_TEAM_MAX");  // (A/B runs: 2 keeps teams of two)
    deal(3);
    {
        const int total = load[0] + load[1] + load[2];
        int least = load[0] < load[1] ? load[0] : load[1];
        least = load[2] < least ? load[2] : least;
        if ((int)roots.size() >= 3 && 6 * least >= total && !(t3 && atoi(t3) < 3) && ch->waves_per_block * 3 <= 16)
            n_team = 3;
        else
            deal(2);
    }
    // worth more wavefronts only when each takes a real share of the work
    if (ok && load[0] > 0 && load[1] > 0 && (n_team == 3 || 5 * (load[0] < load[1] ? load[0] : load[1]) >= load[0] + load[1])) {
        P.team = n_team;
        for (int i = first + 1; i < P.n_ops; ++i) P.ops[i].member = side[find(i)];
        // a workgroup per team: the barrier at the end of a row then holds the two members of one row, not four rows' worth of
        // wavefronts whose walks take different times (DSPEED_HIP_TEAM_WPB: the teams per workgroup, for the A/B)
        int twpb = 1;
        if (const char* tw = getenv("DSPEED_HIP_TEAM_WPB")) twpb = atoi(tw);
        if (twpb >= 1 && twpb < ch->waves_per_block) ch->waves_per_block = P.waves_per_block = twpb;
    }
}

// The interpreter pays a dispatch per op and row (a lone wavefront: op fetch, decode, a few hundred cycles), and a recipe ends in
// dozens of one-lane stores.  Last step, after every shape matcher has read the ops: a run of STORE_SCALARs becomes one op whose lanes
// store one value each, and the no-ops a folded BL_SUBTRACT left are dropped.  (The row-per-lane kernel keeps its plain stores.)
static void merge_scalar_stores(PlanCtx& c) {
    DevProgram& P = c.ch->host;
    if (!c.ch->scalar_ok) {
        int w = 0;
        for (int r = 0; r < P.n_ops;) {
            if (P.ops[r].opcode == DSP_OP_INTERNAL_NOP) {
                ++r;
                continue;
            }
            int e = r;
            while (e < P.n_ops && P.ops[e].opcode == DSP_OP_STORE_SCALAR && e - r < DSP_IC && P.ops[e].member == P.ops[r].member) ++e;
            if (e - r >= 2) {
                DevOp m = P.ops[r];
                m.opcode = DSP_OP_INTERNAL_STORES;
                m.dst = e - r;
                for (int j = 0; j < e - r; ++j) m.ic[j] = P.ops[r + j].io | (P.ops[r + j].ip[0] << 16);
                P.ops[w++] = m;
                r = e;
                continue;
            }
            if (w != r) P.ops[w] = P.ops[r];
            ++w;
            ++r;
        }
        P.n_ops = w;
    }
    for (int i = 0; i < P.n_ops; ++i) P.ops[i].prio = (i * 4) / P.n_ops;
}

// the LDS packing as decided, for dsp_chain_plan and the fuzzer's invariants
static void publish_packing(PlanCtx& c) {
    for (int s = 0; s < c.n_slots; ++s) {
        c.ch->slot_base[s] = c.base[s];
        c.ch->slot_foot[s] = c.foot[s];
        c.ch->slot_first_op[s] = c.first_op[s];
        c.ch->slot_last_op[s] = c.last_op[s];
        c.ch->slot_shares[s] = c.shares[s] ? 1 : 0;
    }
}

int dsp_plan_build(ChainPlan* ch, const dsp_op* ops, int n_ops, const dsp_io_desc* io, int n_io, const int32_t* slot_len, int n_slots,
                   int n_sregs, int compute_dtype) {
    PlanCtx c{ops, n_ops, io, n_io, slot_len, n_slots, n_sregs, compute_dtype, ch};
    if (const int rc = check_call(c)) return rc;
    choose_linear_slots(c);
    slot_lifetimes(c);
    if (const int rc = pack_lds(c)) return rc;  // (slot lengths are checked here: ahead of the bindings, those ahead of the ops)
    pick_waves_per_block(c);
    if (const int rc = bind_io(c)) return rc;
    if (const int rc = lower_ops(c)) return rc;
    fold_load_bl_subtract(c);
    if (c.only) {  // no interpreter op behind it: its own kernel or nothing
        const char* why = "";
        memset(&ch->only, 0, sizeof ch->only);  // once, for whichever block the matcher fills: what it binds nothing to stays null
        ch->n_bound = 0;
        ch->out_vec_at = ch->out_ptr_at = -1;
        if (!c.only->match(c, &why)) return fail(DSP_ERR_UNSUPPORTED, "%s, on rows in memory: %s", c.only->refusal, why);
        if (ch->n_bound > DSP_KERNEL_BINDINGS_MAX)
            return fail(DSP_ERR_UNSUPPORTED, "%s: its shape binds more than %d pointers", c.only->refusal, DSP_KERNEL_BINDINGS_MAX);
        ch->kernel_only = c.only->route;
    }
    match_shapes(c);
    fold_scaled_thresholds(c);
    form_teams(c);
    merge_scalar_stores(c);
    publish_packing(c);
    return DSP_OK;
}

dsp_route dsp_plan_route(const ChainPlan* ch) {
    if (ch && ch->kernel_only != DSP_ROUTE_VM) return ch->kernel_only;  // (whatever the switches say: the interpreter has no such op)
    if (!ch || !ch->fused_on) return DSP_ROUTE_VM;
    if (ch->scalar_ok) return DSP_ROUTE_SCALAR;
    if (ch->pz_ok) return DSP_ROUTE_PZ_ROWS;
    if (ch->red_ok) return DSP_ROUTE_REDUCE;
    if (ch->runs_ok) return DSP_ROUTE_FIR_RUNS;
    if (ch->cur_ok) return DSP_ROUTE_CURRENT;
    if (ch->fir_ok) return ch->fir_f16 ? DSP_ROUTE_FIR_F16 : (ch->fir.store ? DSP_ROUTE_FIR_STORE : DSP_ROUTE_FIR_MFMA);
    if (ch->rows_ok) return DSP_ROUTE_ROWS;
    if (ch->rr_ok && ch->variant != 1) return DSP_ROUTE_ENERGY_RR;
    return ch->fused_ok ? DSP_ROUTE_ENERGY : DSP_ROUTE_VM;
}

int dsp_plan_kernel_only_lds(const ChainPlan* ch) {
    const KernelOnlyRoute* r = ch && ch->kernel_only != DSP_ROUTE_VM ? &kernel_only_routes[ch->kernel_only] : nullptr;
    return r && r->lds ? r->lds(*ch) : 0;
}

void dsp_plan_kernel_only_geometry(const ChainPlan* ch, int64_t n_wf, int* lds_bytes_per_wave, int* waves_per_block, int* blocks) {
    const Geometry g = kernel_only_routes[ch->kernel_only].geometry(*ch, n_wf);
    *lds_bytes_per_wave = g.lds;
    *waves_per_block = g.wpb;
    *blocks = (int)g.blocks;
}

extern "C" void dsp_internal_plan_fill_args(const ChainPlan* ch, void* const* io_ptrs, KernelOnlyArgs* args) {
    char* block = (char*)args;
    memcpy(block, &ch->only, sizeof ch->only);
    for (int k = 0; k < ch->n_bound; ++k) {
        const KernelBinding& b = ch->bound[k];
        if (b.io < 0) continue;
        const DevIO& d = ch->host.io[b.io];
        char* p = (char*)io_ptrs[b.io] + (b.raw ? 0 : (int64_t)d.offset * elem_size(d.dtype));
        memcpy(block + b.at, &p, sizeof p);
    }
    if (ch->out_vec_at >= 0) {  // 16-byte stores: the plan has vouched for the stride, this call's pointer does for the start
        void* out = nullptr;
        memcpy(&out, block + ch->out_ptr_at, sizeof out);
        const int32_t on = out && (reinterpret_cast<uintptr_t>(out) & 15u) == 0 ? 1 : 0;
        memcpy(block + ch->out_vec_at, &on, sizeof on);
    }
}

const char* dsp_plan_route_kernel_name(dsp_route route) {
    return dsp_route_kernel_names[route >= DSP_ROUTE_EXTREMA && route <= DSP_ROUTE_VM ? route : DSP_ROUTE_VM];
}

const char* dsp_plan_kernel_name(const ChainPlan* ch) { return dsp_plan_route_kernel_name(dsp_plan_route(ch)); }

bool dsp_plan_specialised(const ChainPlan* ch) { return ch && (dsp_plan_route(ch) != DSP_ROUTE_VM || (ch->rr_ok && ch->fused_on)); }

extern "C" int dsp_chain_plan(const dsp_op* ops, int n_ops, const dsp_io_desc* io, int n_io, const int32_t* slot_len, int n_slots, int n_sregs,
                              int compute_dtype, dsp_plan_info* info) {
    if (!info) return dsp_fail(DSP_ERR_ARG, "null info");
    memset(info, 0, sizeof *info);
    std::unique_ptr<ChainPlan> ch(new ChainPlan());
    const int rc = dsp_plan_build(ch.get(), ops, n_ops, io, n_io, slot_len, n_slots, n_sregs, compute_dtype);
    if (rc != DSP_OK) return rc;
    snprintf(info->kernel, sizeof info->kernel, "%s", dsp_plan_kernel_name(ch.get()));
    snprintf(info->note, sizeof info->note, "%s", dsp_plan_specialised(ch.get()) ? "" : ch->note.c_str());
    const DevProgram& P = ch->host;
    info->lds_bytes_per_wave = ch->lds_bytes_per_wave;
    info->waves_per_block = ch->waves_per_block;
    info->team = P.team;
    info->n_device_ops = P.n_ops;
    info->lds_elems_per_wave = P.lds_elems_per_wave;
    info->sreg_off = P.sreg_off;
    info->scratch_off = P.scratch_off;
    info->n_slots = P.n_slots;
    for (int s = 0; s < P.n_slots; ++s) {
        info->slot_base[s] = ch->slot_base[s];
        info->slot_elems[s] = ch->slot_foot[s];
        info->slot_first_op[s] = ch->slot_first_op[s];
        info->slot_last_op[s] = ch->slot_last_op[s];
        info->slot_off[s] = P.slots[s].off;
        info->slot_pitch[s] = P.slots[s].pitch;
        info->slot_chunk[s] = P.slots[s].C;
    }
    return DSP_OK;
}
