// pulse_plan_fuzz.cpp -- the planner (dsp_plan.cpp) on programs that hold DSP_OP_PEAK_SNR_THRESHOLD and DSP_OP_MULTI_A_FILTER, with wild
// lengths, list lengths, slots, bindings, offsets, strides and operands: the accepted shapes (the picker alone, the pick-off alone, both in
// one launch with the packed list stored or not) and mutations of them.  A stand-alone program, built with -fsanitize=address,undefined
// (tests/test_pulse_plan_fuzz_cpu.py), as tests/pileup_plan_fuzz.cpp is for the pile-up finder's ops.  Every program is planned or refused; a
// planned one runs on dsp_pulses_kernel with an argument block that names the bindings' geometry and keeps the kernel's bounds.
//   pulse_plan_fuzz <programs> <seed>     prints {"programs": .., "accepted": .., "picker": .., "pickoff": .., "fused": .., "fused_list_stored": ..,
//                                                  "ratio_columns": .., "refused_by_name": .., "refused_shape": .., "refused_long": ..,
//                                                  "refused_width": .., "refused_lengths": .., "refused_return": ..}
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
    const int kind = (int)draw(0, 2);  // 0: the picker, 1: the pick-off, 2: both
    const bool pick = kind != 1, amp = kind != 0, store_list = kind == 0 || chance(50);
    const int32_t m = chance(80) ? (int32_t)draw(1, 64) : (chance(50) ? (int32_t)draw(60, 70) : (int32_t)wild_length());
    const int32_t m_out = chance(92) ? m : (int32_t)wild_length(), m_amp = chance(92) ? m_out : (int32_t)wild_length();
    const int32_t off = chance(60) ? 0 : (int32_t)(chance(90) ? draw(0, 64) : draw(-4, 0x7fffffff));
    int64_t stride = (int64_t)n + off + (chance(50) ? 0 : draw(0, 40));
    if (chance(8)) stride = chance(50) ? draw(-8, 8) : ((int64_t)1 << draw(31, 62));
    const int32_t list_off = chance(70) ? 0 : (int32_t)(chance(90) ? draw(0, 8) : draw(-4, 0x7fffffff));
    int64_t list_stride = (int64_t)m + list_off + (chance(50) ? 0 : draw(0, 9));
    if (chance(8)) list_stride = chance(50) ? draw(-8, 8) : ((int64_t)1 << draw(31, 62));
    auto operand = [&](double usual, int column_percent) {
        dsp_scalar_arg a = {DSP_ARG_CONST, 0, chance(85) ? usual : wild_value()};
        if (chance(column_percent)) {
            p.io.push_back({chance(95) ? DSP_IO_SCALAR_IN : (int)draw(0, 5), chance(92) ? p.dtype : (int)draw(-1, 9), 1, 0, 1});
            a.kind = chance(95) ? DSP_ARG_INPUT : (int)draw(0, 3);
            a.index = (int32_t)p.io.size() - 1;
        }
        return a;
    };
    p.slots = {n, m};
    p.io.push_back({DSP_IO_WF_IN, rows, n, off, stride});                                                      // 0
    p.io.push_back({DSP_IO_WF_IN, chance(92) ? p.dtype : (int)draw(-1, 9), m, list_off, list_stride});  // 1
    p.ops.push_back(make_op(DSP_OP_LOAD, 0, 0, 0));
    p.ops.push_back(make_op(DSP_OP_LOAD, 1, 0, 1));
    if (chance(10)) std::swap(p.ops[0], p.ops[1]);  // (the two loads in either order)
    int list = 1, s_idx = -1, s_amp = -1;
    if (pick) {
        p.slots.push_back(m_out);
        s_idx = (int)p.slots.size() - 1;
        p.n_sregs = chance(95) ? 1 : (int)draw(-1, 3);
        dsp_op o = make_op(DSP_OP_PEAK_SNR_THRESHOLD, s_idx, 0, 0);
        o.ip[0] = 1;
        o.ip[1] = chance(95) ? 0 : (int32_t)draw(-2, 3);
        o.sp[0] = operand(0.8, 30);
        o.sp[1] = operand((double)draw(0, 80), 6);
        p.ops.push_back(o);
        list = s_idx;
    }
    if (amp) {
        p.slots.push_back(m_amp);
        s_amp = (int)p.slots.size() - 1;
        dsp_op o = make_op(DSP_OP_MULTI_A_FILTER, s_amp, chance(95) ? 0 : (int)draw(0, 3), 0);
        o.ip[0] = chance(95) ? list : (int32_t)draw(-1, 4);
        p.ops.push_back(o);
    }
    auto store = [&](int slot, int32_t len) {
        p.io.push_back({DSP_IO_WF_OUT, chance(95) ? p.dtype : (int)draw(-1, 9), len, chance(90) ? 0 : (int32_t)draw(-2, 100), (int64_t)len + (chance(50) ? 0 : draw(0, 9))});
        p.ops.push_back(make_op(DSP_OP_STORE, 0, slot, (int)p.io.size() - 1));
    };
    if (pick && store_list) store(s_idx, m_out);
    if (amp) store(s_amp, m_amp);
    if (pick) {
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
                const int extra[] = {DSP_OP_PEAK_SNR_THRESHOLD, DSP_OP_MULTI_A_FILTER, DSP_OP_MIN_MAX, DSP_OP_BL_SUBTRACT, DSP_OP_STORE, DSP_OP_COPY, DSP_OP_LOAD, DSP_OP_SORT};
                p.ops.insert(p.ops.begin() + draw(0, (int64_t)p.ops.size()), make_op(extra[draw(0, 7)], (int)draw(0, 3), (int)draw(0, 3), (int)draw(0, 3)));
                p.n_sregs = 4;
                break;
            }
            case 6: p.slots.push_back((int32_t)wild_length()); break;
            case 7: p.n_sregs = (int)draw(-1, 70); break;
            default: p.ops[draw(0, (int64_t)p.ops.size() - 1)].opcode = (int32_t)draw(-1, 50); break;
        }
        if (p.ops.empty()) p.ops.push_back(make_op(DSP_OP_MULTI_A_FILTER, 1, 0, 0));
    }
    return p;
}

bool holds_op(const Prog& p) {
    for (const dsp_op& o : p.ops)
        if (o.opcode == DSP_OP_PEAK_SNR_THRESHOLD || o.opcode == DSP_OP_MULTI_A_FILTER) return true;
    return false;
}

bool check(long number, const Prog& p, const ChainPlan& c) {
    if (!holds_op(p)) return true;  // (a mutation took the ops out: any route, tests/planner_fuzz.cpp's business)
    if (c.kernel_only != DSP_ROUTE_PULSES) {
        std::printf("program %ld: holds the op and is planned on route %d\n", number, (int)c.kernel_only);
        return false;
    }
    REQUIRE(dsp_plan_route(&c) == DSP_ROUTE_PULSES);
    REQUIRE(std::strcmp(dsp_plan_kernel_name(&c), "dsp_pulses_kernel") == 0);
    const PulsesArgs& A = c.only.pulses;
    const size_t n_ops = p.ops.size();
    REQUIRE(n_ops >= 4 && n_ops <= 7 && p.ops[0].opcode == DSP_OP_LOAD && p.ops[1].opcode == DSP_OP_LOAD);
    REQUIRE((A.pick == 0 || A.pick == 1) && (A.amp == 0 || A.amp == 1) && (A.pick || A.amp));
    REQUIRE((p.ops[2].opcode == DSP_OP_PEAK_SNR_THRESHOLD) == (A.pick == 1));
    REQUIRE((p.ops[2 + A.pick].opcode == DSP_OP_MULTI_A_FILTER) == (A.amp == 1));
    const dsp_op& first = p.ops[2];
    const dsp_op& ld = p.ops[0].dst == first.src ? p.ops[0] : p.ops[1];
    const dsp_op& lt = &ld == &p.ops[0] ? p.ops[1] : p.ops[0];
    const dsp_io_desc &in = p.io[ld.io], &li = p.io[lt.io];
    REQUIRE(ld.dst == first.src && lt.dst == first.ip[0] && ld.dst != lt.dst);
    REQUIRE(A.len >= 1 && A.len == in.len && A.wf_offset == in.offset && A.wf_stride == in.row_stride);
    REQUIRE(in.offset >= 0 && in.row_stride >= (int64_t)in.offset + in.len);
    REQUIRE(c.only_src.io == ld.io && c.only_src.dtype == in.dtype && c.bound_io(A.list) == lt.io);
    REQUIRE(!c.only_src.vec || ((in.row_stride * dsp_elem_size(in.dtype)) % 16 == 0 && (in.offset * dsp_elem_size(in.dtype)) % 16 == 0 &&
                                  (in.len * dsp_elem_size(in.dtype)) % 16 == 0));
    REQUIRE(p.dtype == DSP_F64 ? in.dtype == DSP_F64 : (in.dtype == DSP_F32 || in.dtype == DSP_I16 || in.dtype == DSP_U16));
    // the kernel's bounds: an entry per lane, the list inside its rows, the width within the row
    REQUIRE(A.m >= 1 && A.m <= DSP_PEAKS_MAX && li.kind == DSP_IO_WF_IN && li.dtype == p.dtype && li.len == A.m && li.offset >= 0);
    REQUIRE(A.list_stride == li.row_stride && A.list_offset == li.offset && li.row_stride >= (int64_t)li.offset + li.len);
    if (A.pick) {
        REQUIRE(A.width >= 0 && A.width <= A.len && c.bound_io(A.n_out) >= 0 && p.io[c.bound_io(A.n_out)].kind == DSP_IO_SCALAR_OUT && p.io[c.bound_io(A.n_out)].dtype == DSP_U32);
        REQUIRE(c.bound_io(A.ratio) < 0 || (p.io[c.bound_io(A.ratio)].kind == DSP_IO_SCALAR_IN && p.io[c.bound_io(A.ratio)].dtype == p.dtype));
        REQUIRE(first.sp[1].kind == DSP_ARG_CONST && first.sp[1].value >= 0 && std::isfinite(first.sp[1].value));
        REQUIRE(A.width == (first.sp[1].value >= A.len ? A.len : (int)first.sp[1].value));
    } else {
        REQUIRE(c.bound_io(A.n_out) < 0 && c.bound_io(A.ratio) < 0 && c.bound_io(A.idx_out) < 0 && A.width == 0);
    }
    if (A.amp) {
        REQUIRE(A.m < A.len && c.bound_io(A.amp_out) >= 0);
        const dsp_io_desc& out = p.io[c.bound_io(A.amp_out)];
        REQUIRE(out.kind == DSP_IO_WF_OUT && out.dtype == p.dtype && out.len == A.m && out.row_stride >= out.len && A.amp_stride == out.row_stride);
    } else {
        REQUIRE(c.bound_io(A.amp_out) < 0 && c.bound_io(A.idx_out) >= 0);
    }
    if (c.bound_io(A.idx_out) >= 0) {
        const dsp_io_desc& out = p.io[c.bound_io(A.idx_out)];
        REQUIRE(A.pick && out.kind == DSP_IO_WF_OUT && out.dtype == p.dtype && out.len == A.m && out.row_stride >= out.len && A.idx_stride == out.row_stride);
        REQUIRE(c.bound_io(A.idx_out) != c.bound_io(A.amp_out));
    }
    // ---- the pointers a launch hands the kernel, from the program: rows and list as they are handed in, the column and the outputs at their
    // first element, null what the program has not
    const dsp_op* pk = A.pick ? &p.ops[2] : nullptr;
    const dsp_op* am = A.amp ? &p.ops[2 + A.pick] : nullptr;
    int idx_io = -1, amp_io = -1;
    for (size_t i = 2 + A.pick + A.amp; i < n_ops; ++i)
        if (p.ops[i].opcode == DSP_OP_STORE) (pk && p.ops[i].src == pk->dst ? idx_io : amp_io) = p.ops[i].io;
    const KernelOnlyArgs launch = launch_args(p, c);
    const PulsesArgs& L = launch.pulses;
    REQUIRE(L.wf == raw_of(ld.io) && L.list == raw_of(lt.io) && L.ratio == first_of(p, pk ? column_of(*pk, 0) : -1));
    REQUIRE(L.idx_out == first_of(p, idx_io) && L.amp_out == first_of(p, am ? amp_io : -1) && L.n_out == first_of(p, pk ? p.ops[n_ops - 1].io : -1));
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const long programs = argc > 1 ? std::atol(argv[1]) : 20000;
    rng.seed(argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 1);
    long accepted = 0, picker = 0, pickoff = 0, fused = 0, fused_list = 0, columns = 0, by_name = 0, shape = 0, too_long = 0, width = 0, lengths = 0, ret = 0;
    for (long number = 0; number < programs; ++number) {
        const Prog p = draw_program();
        const char* why = nullptr;
        const std::unique_ptr<ChainPlan> plan = plan_or_refuse(number, p, &why);
        if (!plan) {
            const bool s = std::strstr(why, "DSP_OP_PEAK_SNR_THRESHOLD / DSP_OP_MULTI_A_FILTER (peak_snr_threshold, multi_a_filter) run on dsp_pulses_kernel only") != nullptr;
            const bool l = std::strstr(why, ": a wavefront keeps one per lane") != nullptr && (std::strstr(why, "candidates") || std::strstr(why, "positions"));
            const bool w = std::strstr(why, "width_in is a") != nullptr;
            const bool x = std::strstr(why, "idx_out has the length of idx_in") != nullptr || std::strstr(why, "va_max_out has the length of vt_maxs_in") != nullptr;
            const bool r = std::strstr(why, "The length of your return array must be smaller than the length of your waveform") != nullptr;
            shape += s, too_long += l, width += w, lengths += x, ret += r;
            if (s || l || w || x || r || std::strstr(why, "PEAK_SNR_THRESHOLD") || std::strstr(why, "MULTI_A_FILTER")) ++by_name;
            continue;
        }
        if (!check(number, p, *plan)) return 1;
        if (holds_op(p) && plan->kernel_only == DSP_ROUTE_PULSES) {
            const PulsesArgs& A = plan->only.pulses;
            ++accepted;
            if (A.pick && A.amp) {
                ++fused;
                fused_list += plan->bound_io(plan->only.pulses.idx_out) >= 0;
            } else {
                ++(A.pick ? picker : pickoff);
            }
            columns += A.pick && plan->bound_io(plan->only.pulses.ratio) >= 0;
        }
    }
    std::printf("{\"programs\": %ld, \"accepted\": %ld, \"picker\": %ld, \"pickoff\": %ld, \"fused\": %ld, \"fused_list_stored\": %ld, \"ratio_columns\": %ld, "
                "\"refused_by_name\": %ld, \"refused_shape\": %ld, \"refused_long\": %ld, \"refused_width\": %ld, \"refused_lengths\": %ld, \"refused_return\": %ld}\n",
                programs, accepted, picker, pickoff, fused, fused_list, columns, by_name, shape, too_long, width, lengths, ret);
    return 0;
}
