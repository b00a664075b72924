// pileup_plan_fuzz.cpp -- the planner (dsp_plan.cpp) on programs that hold DSP_OP_RC_CR2 and DSP_OP_BI_LEVEL_ZERO_CROSSING, with wild lengths,
// list lengths, slots, bindings, offsets, strides and operands: the accepted shapes (the filter alone, the walk alone, both in one launch with
// the filtered row stored or not, each with or without a BL_SUBTRACT behind the LOAD) and mutations of them.  A stand-alone program, built
// with -fsanitize=address,undefined (tests/test_pileup_plan_fuzz_cpu.py), as tests/reflect_plan_fuzz.cpp is for DSP_OP_REFLECTED_CONVOLVE.
// Every program is planned or refused; a planned one runs on dsp_pileup_kernel with an argument block that names the bindings' geometry.
//   pileup_plan_fuzz <programs> <seed>     prints {"programs": .., "accepted": .., "filter": .., "walk": .., "fused": .., "fused_row_stored": ..,
//                                                   "subtracted": .., "columns": .., "refused_by_name": .., "refused_shape": .., "refused_short": ..,
//                                                   "refused_start": .., "refused_lists": ..}
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

double wild_value() {
    switch (draw(0, 9)) {
        case 0: return std::numeric_limits<double>::quiet_NaN();
        case 1: return chance(50) ? INFINITY : -INFINITY;
        case 2: return (double)draw(-3, 3) + 0.5;
        case 3: return (double)draw(-5, 5) * 1e30;
        default: return (double)draw(-3, 300);
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
    const int kind = (int)draw(0, 2);  // 0: the filter, 1: the walk, 2: both
    const bool filter = kind != 1, walk = kind != 0, store_row = kind == 0 || chance(50), subtract = chance(30);
    const int32_t out_len = chance(92) ? n : (int32_t)wild_length();
    int32_t m0 = chance(85) ? (int32_t)draw(1, 40) : (int32_t)wild_length(), m1 = chance(90) ? m0 : (int32_t)wild_length();
    const int32_t off = chance(60) ? 0 : (int32_t)(chance(90) ? draw(0, 64) : draw(-4, 0x7fffffff));
    int64_t stride = (int64_t)n + off + (chance(50) ? 0 : draw(0, 40));
    if (chance(8)) stride = chance(50) ? draw(-8, 8) : ((int64_t)1 << draw(31, 62));
    int64_t out_stride = (int64_t)out_len + (chance(50) ? 0 : draw(0, 40));
    if (chance(8)) out_stride = chance(50) ? draw(-8, 8) : ((int64_t)1 << draw(31, 62));
    auto operand = [&](double usual) {
        dsp_scalar_arg a = {DSP_ARG_CONST, 0, chance(85) ? usual : wild_value()};
        if (chance(25)) {
            p.io.push_back({chance(95) ? DSP_IO_SCALAR_IN : (int)draw(0, 5), chance(92) ? p.dtype : (int)draw(-1, 9), 1, 0, 1});
            a.kind = chance(95) ? DSP_ARG_INPUT : (int)draw(0, 3);
            a.index = (int32_t)p.io.size() - 1;
        }
        return a;
    };
    p.slots = {n};
    p.io.push_back({DSP_IO_WF_IN, rows, n, off, stride});  // 0
    p.ops.push_back(make_op(DSP_OP_LOAD, 0, 0, 0));
    if (subtract) {
        p.ops.push_back(make_op(DSP_OP_BL_SUBTRACT, 0, 0, 0));
        p.ops.back().sp[0] = operand(1000.0);
        p.ops.back().ip[0] = chance(90) ? 0 : 1;
    }
    int src = 0, s_out = -1, s_pol = -1, s_time = -1;
    if (filter) {
        p.slots.push_back(out_len);
        s_out = (int)p.slots.size() - 1;
        p.ops.push_back(make_op(DSP_OP_RC_CR2, s_out, 0, 0));
        p.ops.back().sp[0] = operand(20.0);
        if (chance(85)) p.ops.back().sp[0].kind = DSP_ARG_CONST;
        src = s_out;
    }
    if (walk) {
        p.slots.push_back(m0);
        p.slots.push_back(m1);
        s_pol = (int)p.slots.size() - 2, s_time = s_pol + 1;
        p.n_sregs = chance(95) ? 1 : (int)draw(-1, 3);
        dsp_op o = make_op(DSP_OP_BI_LEVEL_ZERO_CROSSING, s_pol, src, 0);
        o.ip[0] = s_time;
        o.ip[1] = chance(95) ? 0 : (int32_t)draw(-2, 3);
        const double usual[4] = {5.0, -5.0, 100.0, (double)draw(0, n > 1 ? n - 1 : 0)};
        for (int k = 0; k < 4; ++k) o.sp[k] = operand(usual[k]);
        p.ops.push_back(o);
    }
    if (filter && store_row) {
        p.io.push_back({DSP_IO_WF_OUT, chance(92) ? p.dtype : (int)draw(-1, 9), out_len, chance(90) ? 0 : (int32_t)draw(-2, 100), out_stride});
        p.ops.push_back(make_op(DSP_OP_STORE, 0, s_out, (int)p.io.size() - 1));
    }
    if (walk) {
        for (int k = 0; k < 2; ++k) {
            const int32_t len = k ? m1 : m0;
            p.io.push_back({DSP_IO_WF_OUT, chance(95) ? p.dtype : (int)draw(-1, 9), len, 0, (int64_t)len + (chance(50) ? 0 : draw(0, 9))});
            p.ops.push_back(make_op(DSP_OP_STORE, 0, k ? s_time : s_pol, (int)p.io.size() - 1));
        }
        p.io.push_back({DSP_IO_SCALAR_OUT, chance(92) ? DSP_U32 : (int)draw(-1, 9), 1, 0, 1});
        p.ops.push_back(make_op(DSP_OP_STORE_SCALAR, 0, 0, (int)p.io.size() - 1));
        p.ops.back().ip[0] = 0;
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
                const int extra[] = {DSP_OP_RC_CR2, DSP_OP_BI_LEVEL_ZERO_CROSSING, DSP_OP_MIN_MAX, DSP_OP_BL_SUBTRACT, DSP_OP_STORE, DSP_OP_COPY, DSP_OP_LOAD, DSP_OP_SORT};
                p.ops.insert(p.ops.begin() + draw(0, (int64_t)p.ops.size()), make_op(extra[draw(0, 7)], (int)draw(0, 3), (int)draw(0, 3), (int)draw(0, 3)));
                p.n_sregs = 4;
                break;
            }
            case 6: p.slots.push_back((int32_t)wild_length()); break;
            case 7: p.n_sregs = (int)draw(-1, 70); break;
            default: p.ops[draw(0, (int64_t)p.ops.size() - 1)].opcode = (int32_t)draw(-1, 48); break;
        }
        if (p.ops.empty()) p.ops.push_back(make_op(DSP_OP_RC_CR2, 1, 0, 0));
    }
    return p;
}

bool holds_op(const Prog& p) {
    for (const dsp_op& o : p.ops)
        if (o.opcode == DSP_OP_RC_CR2 || o.opcode == DSP_OP_BI_LEVEL_ZERO_CROSSING) return true;
    return false;
}

bool check(long number, const Prog& p, const ChainPlan& c) {
    if (!holds_op(p)) return true;  // (a mutation took the ops out: any route, tests/planner_fuzz.cpp's business)
    if (c.kernel_only != DSP_ROUTE_PILEUP) {
        std::printf("program %ld: holds the op and is planned on route %d\n", number, (int)c.kernel_only);
        return false;
    }
    REQUIRE(dsp_plan_route(&c) == DSP_ROUTE_PILEUP);
    REQUIRE(std::strcmp(dsp_plan_kernel_name(&c), "dsp_pileup_kernel") == 0);
    const PileupArgs& A = c.only.pileup;
    const size_t n_ops = p.ops.size();
    REQUIRE(n_ops >= 3 && n_ops <= 8 && p.ops[0].opcode == DSP_OP_LOAD);
    const size_t first = p.ops[1].opcode == DSP_OP_BL_SUBTRACT ? 2 : 1;
    REQUIRE((A.sub_mode == 1) == (first == 2) && (A.filter == 0 || A.filter == 1) && (A.walk == 0 || A.walk == 1) && (A.filter || A.walk));
    REQUIRE((p.ops[first].opcode == DSP_OP_RC_CR2) == (A.filter == 1));
    REQUIRE((p.ops[first + A.filter].opcode == DSP_OP_BI_LEVEL_ZERO_CROSSING) == (A.walk == 1));
    const dsp_io_desc& in = p.io[p.ops[0].io];
    REQUIRE(A.len >= 1 && A.len == in.len && A.wf_offset == in.offset && A.wf_stride == in.row_stride && (!A.filter || A.len > 3));
    REQUIRE(in.offset >= 0 && in.row_stride >= (int64_t)in.offset + in.len && A.len <= (1 << 24));
    REQUIRE(c.only_src.io == p.ops[0].io && c.only_src.dtype == in.dtype);
    REQUIRE(!c.only_src.vec || ((in.row_stride * dsp_elem_size(in.dtype)) % 16 == 0 && (in.offset * dsp_elem_size(in.dtype)) % 16 == 0 &&
                                  (in.len * dsp_elem_size(in.dtype)) % 16 == 0));
    REQUIRE(p.dtype == DSP_F64 ? in.dtype == DSP_F64 : (in.dtype == DSP_F32 || in.dtype == DSP_I16 || in.dtype == DSP_U16));
    if (A.sub_mode) REQUIRE(c.bound_io(A.sub) < 0 || (p.io[c.bound_io(A.sub)].kind == DSP_IO_SCALAR_IN && p.io[c.bound_io(A.sub)].dtype == p.dtype));
    if (A.filter) {
        REQUIRE(A.tau_nan == 0 || A.tau_nan == 1);
        REQUIRE(A.tau_nan || (A.c1 == A.c1 && A.c2 == A.c2 && A.c3 == A.c3));
    }
    if (c.bound_io(A.out) >= 0) {
        const dsp_io_desc& out = p.io[c.bound_io(A.out)];
        REQUIRE(A.filter && out.kind == DSP_IO_WF_OUT && out.dtype == p.dtype && out.len == A.len && out.row_stride >= out.len && A.out_stride == out.row_stride);
    } else {
        REQUIRE(A.walk);
    }
    if (A.walk) {
        REQUIRE(A.m >= 1 && c.bound_io(A.list[0]) >= 0 && c.bound_io(A.list[1]) >= 0 && c.bound_io(A.list[0]) != c.bound_io(A.list[1]) && c.bound_io(A.n_out) >= 0);
        for (int k = 0; k < 2; ++k) {
            const dsp_io_desc& l = p.io[c.bound_io(A.list[k])];
            REQUIRE(l.kind == DSP_IO_WF_OUT && l.dtype == p.dtype && l.len == A.m && l.row_stride >= l.len && A.list_stride[k] == l.row_stride);
        }
        REQUIRE(p.io[c.bound_io(A.n_out)].kind == DSP_IO_SCALAR_OUT && p.io[c.bound_io(A.n_out)].dtype == DSP_U32);
        for (int k = 0; k < 4; ++k)
            REQUIRE(c.bound_io(A.par[k]) < 0 || (p.io[c.bound_io(A.par[k])].kind == DSP_IO_SCALAR_IN && p.io[c.bound_io(A.par[k])].dtype == p.dtype));
        REQUIRE(c.bound_io(A.par[2]) >= 0 || std::isfinite(A.par_const[2]));  // a constant gate is finite
        if (c.bound_io(A.par[3]) < 0 && A.par_const[3] == A.par_const[3])     // a constant start is integral and inside the row
            REQUIRE(std::floor(A.par_const[3]) == A.par_const[3] && A.par_const[3] >= 0 && A.par_const[3] < A.len);
    } else {
        REQUIRE(c.bound_io(A.list[0]) < 0 && c.bound_io(A.list[1]) < 0 && c.bound_io(A.n_out) < 0 && A.m == 0);
    }
    // ---- the pointers a launch hands the kernel, from the program: the rows as they are handed in, columns and outputs at their first element,
    // null what the program has not; 16-byte stores of the filtered row where its start and stride are whole vectors
    const dsp_op* fi = A.filter ? &p.ops[first] : nullptr;
    const dsp_op* wk = A.walk ? &p.ops[first + A.filter] : nullptr;
    int out_io = -1, list_io[2] = {-1, -1};
    for (size_t i = first + A.filter + A.walk; i < n_ops; ++i) {
        const dsp_op& st = p.ops[i];
        if (st.opcode != DSP_OP_STORE) continue;
        (fi && st.src == fi->dst ? out_io : list_io[st.src == wk->dst ? 0 : 1]) = st.io;
    }
    const KernelOnlyArgs launch = launch_args(p, c);
    const PileupArgs& L = launch.pileup;
    REQUIRE(L.wf == raw_of(p.ops[0].io) && L.sub == first_of(p, first == 2 ? column_of(p.ops[1], 0) : -1) && L.out == first_of(p, out_io));
    REQUIRE(L.list[0] == first_of(p, list_io[0]) && L.list[1] == first_of(p, list_io[1]) && L.n_out == first_of(p, wk ? p.ops[n_ops - 1].io : -1));
    for (int k = 0; k < 4; ++k) REQUIRE(L.par[k] == first_of(p, wk ? column_of(*wk, k) : -1));
    REQUIRE(L.out_vec == vector_store(p, out_io, p.dtype == DSP_F64 ? 8 : 4));
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const long programs = argc > 1 ? std::atol(argv[1]) : 20000;
    rng.seed(argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 1);
    long accepted = 0, filter = 0, walk = 0, fused = 0, fused_row = 0, subtracted = 0, columns = 0, by_name = 0, shape = 0, too_short = 0, start = 0, lists = 0;
    for (long number = 0; number < programs; ++number) {
        const Prog p = draw_program();
        const char* why = nullptr;
        const std::unique_ptr<ChainPlan> plan = plan_or_refuse(number, p, &why);
        if (!plan) {
            const bool s = std::strstr(why, "DSP_OP_RC_CR2 / DSP_OP_BI_LEVEL_ZERO_CROSSING (rc_cr2, bi_level_zero_crossing_time_points) run on dsp_pileup_kernel only") != nullptr;
            const bool l = std::strstr(why, "The length of the waveform must be larger than 3") != nullptr;
            const bool t = std::strstr(why, "The starting index") != nullptr;
            const bool x = std::strstr(why, "the output arrays are of different lengths") != nullptr || std::strstr(why, "hold at least one entry") != nullptr;
            shape += s, too_short += l, start += t, lists += x;
            if (s || l || t || x || std::strstr(why, "rc_cr2") || std::strstr(why, "bi_level_zero_crossing_time_points") || std::strstr(why, "RC_CR2") ||
                std::strstr(why, "BI_LEVEL_ZERO_CROSSING"))
                ++by_name;
            continue;
        }
        if (!check(number, p, *plan)) return 1;
        if (holds_op(p)) {
            const PileupArgs& A = plan->only.pileup;
            ++accepted;
            if (A.filter && A.walk) {
                ++fused;
                fused_row += plan->bound_io(plan->only.pileup.out) >= 0;
            } else {
                ++(A.filter ? filter : walk);
            }
            subtracted += A.sub_mode;
            for (int k = 0; k < 4; ++k) columns += A.walk && plan->bound_io(plan->only.pileup.par[k]) >= 0;
        }
    }
    std::printf("{\"programs\": %ld, \"accepted\": %ld, \"filter\": %ld, \"walk\": %ld, \"fused\": %ld, \"fused_row_stored\": %ld, \"subtracted\": %ld, "
                "\"columns\": %ld, \"refused_by_name\": %ld, \"refused_shape\": %ld, \"refused_short\": %ld, \"refused_start\": %ld, \"refused_lists\": %ld}\n",
                programs, accepted, filter, walk, fused, fused_row, subtracted, columns, by_name, shape, too_short, start, lists);
    return 0;
}
