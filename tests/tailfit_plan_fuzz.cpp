// tailfit_plan_fuzz.cpp -- the planner (dsp_plan.cpp) on programs that hold DSP_OP_LOG_CHECK, DSP_OP_POLY_FIT, DSP_OP_POLY_DIFF and
// DSP_OP_POLY_EXP_RMS, with wild lengths, numbers of coefficients, slots, bindings, offsets and strides: the accepted shapes (each processor
// alone, log_check -> poly_fit, [log_check ->] poly_fit -> the residuals with the logged row and the coefficients stored or not, each with or
// without a BL_SUBTRACT behind the LOAD) and mutations of them.  A stand-alone program, built with -fsanitize=address,undefined
// (tests/test_tailfit_plan_fuzz_cpu.py), as tests/pileup_plan_fuzz.cpp is for the pile-up finder's ops.  Every program is planned or
// refused; a planned one runs on dsp_tailfit_kernel with an argument block that names the bindings' geometry.
//   tailfit_plan_fuzz <programs> <seed>     prints {"programs": .., "accepted": .., "log": .., "fit": .., "resid": .., "log_fit": .., "chain": ..,
//                                                    "log_stored": .., "pars_stored": .., "subtracted": .., "refused_by_name": .., "refused_shape": ..,
//                                                    "refused_many": .., "refused_power": ..}
#include <cmath>
#include <limits>
#include "plan_fuzz.h"

namespace {

int64_t wild_length() {
    switch (draw(0, 9)) {
        case 0: return draw(-3, 5);
        case 1: return (int64_t)1 << draw(0, 25);
        case 2: return ((int64_t)1 << draw(0, 25)) + draw(-1, 1);
        case 3: return draw(60, 70);
        case 4: return draw(1 << 20, (1 << 20) + 2);
        case 5: return 0x7fffffff - draw(0, 3);
        default: return draw(1, 20000);
    }
}

Prog draw_program() {
    Prog p;
    p.dtype = chance(35) ? DSP_F64 : DSP_F32;
    const int rows_f32[] = {DSP_F32, DSP_I16, DSP_U16}, rows_f64[] = {DSP_F64, DSP_F64, DSP_I32};
    int rows = p.dtype == DSP_F64 ? rows_f64[draw(0, 2)] : rows_f32[draw(0, 2)];
    if (chance(5)) rows = (int)draw(-1, 9);
    int32_t n = (int32_t)wild_length();
    if (chance(70)) n = (int32_t)draw(1, 9000);
    // 0: log_check, 1: poly_fit, 2: the residuals of coefficients from memory, 3: log_check -> poly_fit, 4: [log_check ->] poly_fit -> the residuals
    const int kind = (int)draw(0, 4);
    const bool log = kind == 0 || kind == 3 || (kind == 4 && chance(75)), fit = kind == 1 || kind >= 3, resid = kind == 2 || kind == 4;
    const bool store_log = log && (!fit || chance(50)), store_pars = fit && (!resid || chance(50)), subtract = chance(30);
    const int32_t out_len = chance(92) ? n : (int32_t)wild_length();
    const int32_t m = chance(85) ? (int32_t)draw(1, 8) : (chance(50) ? (int32_t)draw(9, 12) : (int32_t)wild_length());
    const int32_t off = chance(60) ? 0 : (int32_t)(chance(90) ? draw(0, 64) : draw(-4, 0x7fffffff));
    int64_t stride = (int64_t)n + off + (chance(50) ? 0 : draw(0, 40));
    if (chance(8)) stride = chance(50) ? draw(-8, 8) : ((int64_t)1 << draw(31, 62));
    int64_t out_stride = (int64_t)out_len + (chance(50) ? 0 : draw(0, 40));
    if (chance(8)) out_stride = chance(50) ? draw(-8, 8) : ((int64_t)1 << draw(31, 62));
    p.slots = {n};
    p.io.push_back({DSP_IO_WF_IN, rows, n, off, stride});  // 0
    p.ops.push_back(make_op(DSP_OP_LOAD, 0, 0, 0));
    int s_pars = -1, s_log = -1;
    if (resid && !fit) {
        p.slots.push_back(m);
        s_pars = (int)p.slots.size() - 1;
        p.io.push_back({DSP_IO_WF_IN, chance(92) ? p.dtype : (int)draw(-1, 9), chance(95) ? m : (int32_t)wild_length(), chance(90) ? 0 : (int32_t)draw(-2, 9),
                        (int64_t)m + (chance(50) ? 0 : draw(0, 9))});
        p.ops.push_back(make_op(DSP_OP_LOAD, s_pars, 0, (int)p.io.size() - 1));
    }
    if (subtract) {
        dsp_op o = make_op(DSP_OP_BL_SUBTRACT, 0, 0, 0);
        o.sp[0] = {DSP_ARG_CONST, 0, 1000.0};
        if (chance(40)) {
            p.io.push_back({chance(95) ? DSP_IO_SCALAR_IN : (int)draw(0, 5), chance(92) ? p.dtype : (int)draw(-1, 9), 1, 0, 1});
            o.sp[0].kind = chance(95) ? DSP_ARG_INPUT : (int)draw(0, 3);
            o.sp[0].index = (int32_t)p.io.size() - 1;
        }
        o.ip[0] = chance(90) ? 0 : 1;
        if (chance(50) || p.ops.size() == 1) p.ops.push_back(o);
        else p.ops.insert(p.ops.begin() + 1, o);  // (ahead of the LOAD of the coefficients)
    }
    int src = 0;
    if (log) {
        p.slots.push_back(out_len);
        s_log = (int)p.slots.size() - 1;
        p.ops.push_back(make_op(DSP_OP_LOG_CHECK, s_log, 0, 0));
        src = s_log;
    }
    if (fit) {
        p.slots.push_back(m);
        s_pars = (int)p.slots.size() - 1;
        const int64_t mm = (int64_t)m * m;
        p.io.push_back({chance(95) ? DSP_IO_TAPS : (int)draw(0, 5), chance(92) ? DSP_F64 : (int)draw(-1, 9), chance(92) && mm > 0 && mm < (1 << 28) ? (int32_t)mm : (int32_t)wild_length(), 0, 0});
        p.ops.push_back(make_op(DSP_OP_POLY_FIT, s_pars, src, (int)p.io.size() - 1));
    }
    if (resid) {
        p.n_sregs = chance(95) ? 2 : (int)draw(-1, 3);
        dsp_op o = make_op(chance(50) ? DSP_OP_POLY_DIFF : DSP_OP_POLY_EXP_RMS, chance(95) ? 0 : (int)draw(-2, 3), log && chance(50) ? s_log : 0, 0);
        o.ip[0] = s_pars;
        p.ops.push_back(o);
    }
    if (store_log) {
        p.io.push_back({DSP_IO_WF_OUT, chance(92) ? p.dtype : (int)draw(-1, 9), out_len, chance(90) ? 0 : (int32_t)draw(-2, 100), out_stride});
        p.ops.push_back(make_op(DSP_OP_STORE, 0, s_log, (int)p.io.size() - 1));
    }
    if (store_pars) {
        p.io.push_back({DSP_IO_WF_OUT, chance(95) ? p.dtype : (int)draw(-1, 9), m, 0, (int64_t)m + (chance(50) ? 0 : draw(0, 9))});
        p.ops.push_back(make_op(DSP_OP_STORE, 0, s_pars, (int)p.io.size() - 1));
    }
    if (resid)
        for (int k = 0; k < 2; ++k) {
            p.io.push_back({DSP_IO_SCALAR_OUT, chance(92) ? p.dtype : (int)draw(-1, 9), 1, 0, 1});
            p.ops.push_back(make_op(DSP_OP_STORE_SCALAR, 0, 0, (int)p.io.size() - 1));
            p.ops.back().ip[0] = chance(95) ? k : (int32_t)draw(-1, 3);
        }
    // mutations: a wild field, an op more or less, a slot more, registers
    for (int k = (int)draw(0, 3); k > 0 && chance(45); --k) {
        switch (draw(0, 8)) {
            case 0: p.ops[draw(0, (int64_t)p.ops.size() - 1)].dst = (int32_t)draw(-2, 5); break;
            case 1: p.ops[draw(0, (int64_t)p.ops.size() - 1)].src = (int32_t)draw(-2, 5); break;
            case 2: p.ops[draw(0, (int64_t)p.ops.size() - 1)].io = (int32_t)draw(-2, 9); break;
            case 3: p.ops[draw(0, (int64_t)p.ops.size() - 1)].ip[draw(0, 3)] = (int32_t)draw(-3, 70000); break;
            case 4: p.ops.erase(p.ops.begin() + draw(0, (int64_t)p.ops.size() - 1)); break;
            case 5: {
                const int extra[] = {DSP_OP_LOG_CHECK, DSP_OP_POLY_FIT, DSP_OP_POLY_DIFF, DSP_OP_POLY_EXP_RMS, DSP_OP_MIN_MAX, DSP_OP_BL_SUBTRACT, DSP_OP_STORE, DSP_OP_LOAD};
                p.ops.insert(p.ops.begin() + draw(0, (int64_t)p.ops.size()), make_op(extra[draw(0, 7)], (int)draw(0, 3), (int)draw(0, 3), (int)draw(0, 3)));
                p.n_sregs = 4;
                break;
            }
            case 6: p.slots.push_back((int32_t)wild_length()); break;
            case 7: p.n_sregs = (int)draw(-1, 70); break;
            default: p.ops[draw(0, (int64_t)p.ops.size() - 1)].opcode = (int32_t)draw(-1, 54); break;
        }
        if (p.ops.empty()) p.ops.push_back(make_op(DSP_OP_LOG_CHECK, 1, 0, 0));
    }
    return p;
}

bool is_mine(int opcode) { return opcode >= DSP_OP_LOG_CHECK && opcode <= DSP_OP_POLY_EXP_RMS; }
bool holds_op(const Prog& p) {
    for (const dsp_op& o : p.ops)
        if (is_mine(o.opcode)) return true;
    return false;
}

bool check(long number, const Prog& p, const ChainPlan& c) {
    if (!holds_op(p)) return true;  // (a mutation took the ops out: any route, tests/planner_fuzz.cpp's business)
    if (c.kernel_only != DSP_ROUTE_TAILFIT) {
        std::printf("program %ld: holds the op and is planned on route %d\n", number, (int)c.kernel_only);
        return false;
    }
    REQUIRE(dsp_plan_route(&c) == DSP_ROUTE_TAILFIT);
    REQUIRE(std::strcmp(dsp_plan_kernel_name(&c), "dsp_tailfit_kernel") == 0);
    const TailfitArgs& A = c.only.tailfit;
    const size_t n_ops = p.ops.size();
    REQUIRE(n_ops >= 3 && n_ops <= 9 && p.ops[0].opcode == DSP_OP_LOAD);
    int count[4] = {0, 0, 0, 0}, subs = 0, loads = 0;
    for (const dsp_op& o : p.ops) {
        if (is_mine(o.opcode)) ++count[o.opcode - DSP_OP_LOG_CHECK];
        subs += o.opcode == DSP_OP_BL_SUBTRACT, loads += o.opcode == DSP_OP_LOAD;
    }
    REQUIRE(count[0] == A.log && count[1] == A.fit && count[2] == (A.resid == 1) && count[3] == (A.resid == 2) && subs == A.sub_mode);
    REQUIRE((A.log == 0 || A.log == 1) && (A.fit == 0 || A.fit == 1) && A.resid >= 0 && A.resid <= 2 && (A.log || A.fit || A.resid));
    REQUIRE(!(A.log && A.resid && !A.fit) && (!A.resid_log || A.log) && loads == 1 + (A.resid && !A.fit ? 1 : 0));
    const dsp_io_desc& in = p.io[c.only_src.io];
    REQUIRE(in.kind == DSP_IO_WF_IN && A.len >= 1 && A.len == in.len && A.wf_offset == in.offset && A.wf_stride == in.row_stride);
    REQUIRE(in.offset >= 0 && in.row_stride >= (int64_t)in.offset + in.len && c.only_src.dtype == in.dtype);
    REQUIRE(!c.only_src.vec || ((in.row_stride * dsp_elem_size(in.dtype)) % 16 == 0 && (in.offset * dsp_elem_size(in.dtype)) % 16 == 0 &&
                                   (in.len * dsp_elem_size(in.dtype)) % 16 == 0));
    REQUIRE(p.dtype == DSP_F64 ? in.dtype == DSP_F64 : (in.dtype == DSP_F32 || in.dtype == DSP_I16 || in.dtype == DSP_U16));
    if (A.sub_mode) REQUIRE(c.bound_io(A.sub) < 0 || (p.io[c.bound_io(A.sub)].kind == DSP_IO_SCALAR_IN && p.io[c.bound_io(A.sub)].dtype == p.dtype));
    if (A.fit || A.resid) REQUIRE(A.m >= 1 && A.m <= DSP_POLY_MAX && dsp_poly_powers_fit(A.len, A.m));
    if (A.fit) {
        REQUIRE(c.bound_io(A.inv) >= 0 && c.bound_io(A.pars) < 0);
        const dsp_io_desc& inv = p.io[c.bound_io(A.inv)];
        REQUIRE(inv.kind == DSP_IO_TAPS && inv.dtype == DSP_F64 && inv.len == A.m * A.m);
    } else {
        REQUIRE(c.bound_io(A.inv) < 0 && c.bound_io(A.pars_out) < 0);
    }
    if (A.resid && !A.fit) {
        REQUIRE(c.bound_io(A.pars) >= 0);
        const dsp_io_desc& pars = p.io[c.bound_io(A.pars)];
        REQUIRE(pars.kind == DSP_IO_WF_IN && pars.dtype == p.dtype && pars.len == A.m && pars.offset >= 0 && pars.row_stride >= (int64_t)pars.offset + pars.len);
        REQUIRE(A.pars_stride == pars.row_stride && A.pars_offset == pars.offset);
    }
    if (c.bound_io(A.out) >= 0) {
        const dsp_io_desc& out = p.io[c.bound_io(A.out)];
        REQUIRE(A.log && out.kind == DSP_IO_WF_OUT && out.dtype == p.dtype && out.len == A.len && out.row_stride >= out.len && A.out_stride == out.row_stride);
    } else {
        REQUIRE(!A.log || A.fit);
    }
    if (c.bound_io(A.pars_out) >= 0) {
        const dsp_io_desc& out = p.io[c.bound_io(A.pars_out)];
        REQUIRE(A.fit && out.kind == DSP_IO_WF_OUT && out.dtype == p.dtype && out.len == A.m && out.row_stride >= out.len && A.pars_out_stride == out.row_stride);
        REQUIRE(c.bound_io(A.pars_out) != c.bound_io(A.out));
    } else {
        REQUIRE(!A.fit || A.resid);
    }
    if (A.resid) {
        REQUIRE(c.bound_io(A.mean_out) >= 0 && c.bound_io(A.rms_out) >= 0 && c.bound_io(A.mean_out) != c.bound_io(A.rms_out));
        for (int k : {c.bound_io(A.mean_out), c.bound_io(A.rms_out)}) REQUIRE(p.io[k].kind == DSP_IO_SCALAR_OUT && p.io[k].dtype == p.dtype);
    } else {
        REQUIRE(c.bound_io(A.mean_out) < 0 && c.bound_io(A.rms_out) < 0);
    }
    // ---- the pointers a launch hands the kernel, from the program: rows and loaded coefficients as they are handed in, column, matrix and outputs
    // at their first element, null what the program has not; 16-byte stores of the logged row where its start and stride are whole vectors
    const dsp_op *lg = nullptr, *ft = nullptr, *rs = nullptr, *bs = nullptr;
    for (const dsp_op& o : p.ops) {
        if (o.opcode == DSP_OP_LOG_CHECK) lg = &o;
        if (o.opcode == DSP_OP_POLY_FIT) ft = &o;
        if (o.opcode == DSP_OP_POLY_DIFF || o.opcode == DSP_OP_POLY_EXP_RMS) rs = &o;
        if (o.opcode == DSP_OP_BL_SUBTRACT) bs = &o;
    }
    const dsp_op& first = lg ? *lg : (ft ? *ft : *rs);
    int rows_io = -1, pars_io = -1, out_io = -1, pars_out_io = -1, mean_io = -1, rms_io = -1;
    for (const dsp_op& o : p.ops) {
        if (o.opcode == DSP_OP_LOAD) (o.dst == first.src ? rows_io : pars_io) = o.io;
        if (o.opcode == DSP_OP_STORE) (lg && o.src == lg->dst ? out_io : pars_out_io) = o.io;
        if (o.opcode == DSP_OP_STORE_SCALAR) (o.ip[0] == rs->dst ? mean_io : rms_io) = o.io;
    }
    const KernelOnlyArgs launch = launch_args(p, c);
    const TailfitArgs& L = launch.tailfit;
    REQUIRE(L.wf == raw_of(rows_io) && L.pars == raw_of(pars_io) && L.sub == first_of(p, bs ? column_of(*bs, 0) : -1) && L.inv == first_of(p, ft ? ft->io : -1));
    REQUIRE(L.out == first_of(p, out_io) && L.pars_out == first_of(p, pars_out_io) && L.mean_out == first_of(p, mean_io) && L.rms_out == first_of(p, rms_io));
    REQUIRE(L.out_vec == vector_store(p, out_io, p.dtype == DSP_F64 ? 8 : 4));
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const long programs = argc > 1 ? std::atol(argv[1]) : 20000;
    rng.seed(argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 1);
    long accepted = 0, log = 0, fit = 0, resid = 0, log_fit = 0, chain = 0, log_stored = 0, pars_stored = 0, subtracted = 0, by_name = 0, shape = 0, many = 0, power = 0;
    for (long number = 0; number < programs; ++number) {
        const Prog p = draw_program();
        const char* why = nullptr;
        const std::unique_ptr<ChainPlan> plan = plan_or_refuse(number, p, &why);
        if (!plan) {
            const bool s = std::strstr(why, "(log_check, poly_fit, poly_diff, poly_exp_rms) run on dsp_tailfit_kernel only") != nullptr;
            const bool c = std::strstr(why, "a lane keeps one float64 accumulator each") != nullptr;
            const bool w = std::strstr(why, "int64 power i**j wraps silently") != nullptr;
            shape += s, many += c, power += w;
            if (s || c || w || std::strstr(why, "log_check") || std::strstr(why, "poly_fit") || std::strstr(why, "LOG_CHECK") || std::strstr(why, "POLY_"))
                ++by_name;
            continue;
        }
        if (!check(number, p, *plan)) return 1;
        if (holds_op(p)) {
            const TailfitArgs& A = plan->only.tailfit;
            ++accepted;
            if (A.fit && A.resid) ++chain;
            else if (A.log && A.fit) ++log_fit;
            else ++(A.log ? log : (A.fit ? fit : resid));
            log_stored += A.fit && plan->bound_io(plan->only.tailfit.out) >= 0;
            pars_stored += A.resid && plan->bound_io(plan->only.tailfit.pars_out) >= 0;
            subtracted += A.sub_mode;
        }
    }
    std::printf("{\"programs\": %ld, \"accepted\": %ld, \"log\": %ld, \"fit\": %ld, \"resid\": %ld, \"log_fit\": %ld, \"chain\": %ld, \"log_stored\": %ld, "
                "\"pars_stored\": %ld, \"subtracted\": %ld, \"refused_by_name\": %ld, \"refused_shape\": %ld, \"refused_many\": %ld, \"refused_power\": %ld}\n",
                programs, accepted, log, fit, resid, log_fit, chain, log_stored, pars_stored, subtracted, by_name, shape, many, power);
    return 0;
}
