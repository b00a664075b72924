// reflect_plan_fuzz.cpp -- the planner (dsp_plan.cpp) on programs that hold DSP_OP_REFLECTED_CONVOLVE, with wild lengths, tap counts, slots,
// bindings, offsets and strides: the two accepted shapes (the filter alone; with an avg_current of the filtered row, that row stored or
// not) and mutations of them.  A stand-alone program, built with -fsanitize=address,undefined (tests/test_reflect_plan_fuzz_cpu.py), as
// tests/interp_plan_fuzz.cpp is for DSP_OP_INTERP_UPSAMPLE.  Every program is planned or refused; a planned one runs on dsp_reflect_kernel
// with an argument block that names the bindings' geometry and an LDS footprint that fits.
//   reflect_plan_fuzz <programs> <seed>     prints {"programs": .., "accepted": .., "plain": .., "fused": .., "fused_row_stored": .., "narrow": ..,
//                                                    "wide": .., "refused_by_name": .., "refused_shape": .., "refused_long": .., "refused_limit": ..}
#include "plan_fuzz.h"

namespace {

int64_t wild_length() {
    switch (draw(0, 9)) {
        case 0: return draw(-3, 3);
        case 1: return (int64_t)1 << draw(0, 21);
        case 2: return ((int64_t)1 << draw(0, 21)) + draw(-1, 1);
        case 3: return draw(16370, 16390);
        case 4: return draw(8180, 8196);
        case 5: return chance(50) ? draw(2030, 2056) : draw(1010, 1030);
        case 6: return 0x7fffffff - draw(0, 3);
        default: return draw(1, 20000);
    }
}

Prog draw_program() {
    Prog p;
    p.dtype = chance(35) ? DSP_F64 : DSP_F32;
    const int rows_f32[] = {DSP_F32, DSP_I16, DSP_U16}, rows_f64[] = {DSP_F64, DSP_F64, DSP_I32};
    int rows = p.dtype == DSP_F64 ? rows_f64[draw(0, 2)] : rows_f32[draw(0, 2)];
    if (chance(5)) rows = (int)draw(-1, 9);
    const int lim = p.dtype == DSP_F64 ? 8192 : 16384;
    int32_t n = (int32_t)wild_length();
    if (chance(70)) n = (int32_t)draw(1, lim);
    int32_t m = (int32_t)wild_length();
    if (chance(75) && n > 0) m = (int32_t)(chance(60) ? draw(1, n < 300 ? n : 300) : chance(50) ? draw(1, n) : (int64_t)lim + 1 - n + draw(-2, 2));
    const bool fused = chance(50);
    const bool store_row = !fused || chance(50);
    double length = chance(85) ? (double)draw(1, n > 1 && n < 100000 ? (n - 1 < 40 ? n - 1 : 40) : 1) : (double)draw(-3, 70000);
    if (chance(10)) length += 0.5;
    const int32_t lag = (int32_t)length;
    const int32_t nc = chance(92) ? n - lag : (int32_t)wild_length();
    const int32_t off = chance(60) ? 0 : (int32_t)(chance(90) ? draw(0, 64) : draw(-4, 0x7fffffff));
    int64_t stride = (int64_t)n + off + (chance(50) ? 0 : draw(0, 40));
    if (chance(8)) stride = chance(50) ? draw(-8, 8) : ((int64_t)1 << draw(31, 62));
    int64_t out_stride = (int64_t)n + (chance(50) ? 0 : draw(0, 40));
    if (chance(8)) out_stride = chance(50) ? draw(-8, 8) : ((int64_t)1 << draw(31, 62));
    const int32_t out_len = chance(92) ? n : (int32_t)wild_length();
    p.slots = {n, out_len};
    p.io.push_back({DSP_IO_WF_IN, rows, n, off, stride});                                                                    // 0
    p.io.push_back({chance(95) ? DSP_IO_TAPS : (int)draw(0, 5), chance(92) ? p.dtype : (int)draw(-1, 9), m, 0, 0});          // 1
    p.io.push_back({DSP_IO_WF_OUT, chance(92) ? p.dtype : (int)draw(-1, 9), out_len, chance(90) ? 0 : (int32_t)draw(-2, 100), out_stride});  // 2
    p.ops.push_back(make_op(DSP_OP_LOAD, 0, 0, 0));
    p.ops.push_back(make_op(DSP_OP_REFLECTED_CONVOLVE, 1, 0, 1));
    p.ops.back().ip[0] = chance(85) ? 0 : (int32_t)draw(-2, 3);
    if (fused) {
        p.slots.push_back(nc);
        p.io.push_back({DSP_IO_WF_OUT, chance(95) ? p.dtype : (int)draw(-1, 9), nc, 0, (int64_t)nc + (chance(50) ? 0 : draw(0, 9))});  // 3
        p.ops.push_back(make_op(DSP_OP_AVG_CURRENT, 2, 1, 0));
        p.ops.back().sp[0] = {chance(95) ? DSP_ARG_CONST : (int)draw(0, 3), 0, length};
        if (store_row && chance(50)) p.ops.push_back(make_op(DSP_OP_STORE, 0, 1, 2));
        p.ops.push_back(make_op(DSP_OP_STORE, 0, 2, 3));
        if (store_row && p.ops.size() == 4) p.ops.push_back(make_op(DSP_OP_STORE, 0, 1, 2));
    } else {
        p.ops.push_back(make_op(DSP_OP_STORE, 0, 1, 2));
    }
    // mutations: a wild field, an op more or less, a slot more, registers
    for (int k = (int)draw(0, 3); k > 0 && chance(45); --k) {
        switch (draw(0, 8)) {
            case 0: p.ops[draw(0, (int64_t)p.ops.size() - 1)].dst = (int32_t)draw(-2, 5); break;
            case 1: p.ops[draw(0, (int64_t)p.ops.size() - 1)].src = (int32_t)draw(-2, 5); break;
            case 2: p.ops[draw(0, (int64_t)p.ops.size() - 1)].io = (int32_t)draw(-2, 5); break;
            case 3: p.ops[draw(0, (int64_t)p.ops.size() - 1)].ip[draw(0, 3)] = (int32_t)draw(-3, 70000); break;
            case 4: p.ops.erase(p.ops.begin() + draw(0, (int64_t)p.ops.size() - 1)); break;
            case 5: {
                const int extra[] = {DSP_OP_REFLECTED_CONVOLVE, DSP_OP_MIN_MAX, DSP_OP_BL_SUBTRACT, DSP_OP_STORE, DSP_OP_AVG_CURRENT, DSP_OP_COPY, DSP_OP_LOAD, DSP_OP_SORT};
                p.ops.insert(p.ops.begin() + draw(0, (int64_t)p.ops.size()), make_op(extra[draw(0, 7)], (int)draw(0, 2), (int)draw(0, 2), (int)draw(0, 3)));
                p.n_sregs = 4;
                break;
            }
            case 6: p.slots.push_back((int32_t)wild_length()); break;
            case 7: p.n_sregs = (int)draw(-1, 70); break;
            default: p.ops[draw(0, (int64_t)p.ops.size() - 1)].opcode = (int32_t)draw(-1, 46); break;
        }
        if (p.ops.empty()) p.ops.push_back(make_op(DSP_OP_REFLECTED_CONVOLVE, 1, 0, 1));
    }
    return p;
}

bool holds_op(const Prog& p) {
    for (const dsp_op& o : p.ops)
        if (o.opcode == DSP_OP_REFLECTED_CONVOLVE) return true;
    return false;
}

bool check(long number, const Prog& p, const ChainPlan& c) {
    if (!holds_op(p)) return true;  // (a mutation took the op out: any route, tests/planner_fuzz.cpp's business)
    if (c.kernel_only != DSP_ROUTE_REFLECT) {  // (a mutation put an op of an earlier kernel-only route in as well and the program has that shape: impossible)
        std::printf("program %ld: holds the op and is planned on route %d\n", number, (int)c.kernel_only);
        return false;
    }
    REQUIRE(dsp_plan_route(&c) == DSP_ROUTE_REFLECT);
    REQUIRE(std::strcmp(dsp_plan_kernel_name(&c), "dsp_reflect_kernel") == 0);
    const size_t n_ops = p.ops.size();
    REQUIRE(n_ops >= 3 && n_ops <= 5 && p.ops[0].opcode == DSP_OP_LOAD && p.ops[1].opcode == DSP_OP_REFLECTED_CONVOLVE);
    const bool fused = p.ops[2].opcode == DSP_OP_AVG_CURRENT;
    for (size_t i = fused ? 3 : 2; i < n_ops; ++i) REQUIRE(p.ops[i].opcode == DSP_OP_STORE);
    REQUIRE(n_ops == (fused ? 4u : 3u) || (fused && n_ops == 5));
    const ReflectArgs& A = c.only.reflect;
    const dsp_io_desc &in = p.io[p.ops[0].io], &taps = p.io[p.ops[1].io];
    const int esz = p.dtype == DSP_F64 ? 8 : 4;
    REQUIRE(A.len >= 1 && A.n_taps >= 1 && A.n_taps <= A.len && dsp_reflect::fits(A.len, A.n_taps, esz));
    REQUIRE(A.len == in.len && A.wf_offset == in.offset && A.wf_stride == in.row_stride && A.n_taps == taps.len);
    REQUIRE(taps.kind == DSP_IO_TAPS && taps.dtype == p.dtype && c.bound_io(A.taps) == p.ops[1].io);
    REQUIRE(in.offset >= 0 && in.row_stride >= (int64_t)in.offset + in.len);
    REQUIRE(A.wide == (dsp_reflect::wide(A.len, A.n_taps, esz) ? 1 : 0) && (A.taps_nan == 0 || A.taps_nan == 1));
    REQUIRE(dsp_reflect::lds_bytes(A.len, A.n_taps, esz) <= 64 * 1024 + 32 + 16 && dsp_reflect::row_bytes(A.len, A.n_taps, esz) >= dsp_reflect::staged(A.len, A.n_taps) * esz);
    REQUIRE(c.only_src.io == p.ops[0].io && c.only_src.dtype == in.dtype);
    REQUIRE(!c.only_src.vec || ((in.row_stride * dsp_elem_size(in.dtype)) % 16 == 0 && (in.offset * dsp_elem_size(in.dtype)) % 16 == 0 &&
                                   (in.len * dsp_elem_size(in.dtype)) % 16 == 0));
    if (c.bound_io(A.out) >= 0) {
        const dsp_io_desc& out = p.io[c.bound_io(A.out)];
        REQUIRE(out.kind == DSP_IO_WF_OUT && out.dtype == p.dtype && out.len == A.len && out.row_stride >= out.len && A.out_stride == out.row_stride);
    }
    if (fused) {
        REQUIRE(c.bound_io(A.cur) >= 0 && A.lag >= 1 && A.lag < A.len && A.lag == (int)A.length && A.length >= 1.0);
        const dsp_io_desc& cur = p.io[c.bound_io(A.cur)];
        REQUIRE(cur.kind == DSP_IO_WF_OUT && cur.dtype == p.dtype && cur.len == A.len - A.lag && cur.row_stride >= cur.len && A.cur_stride == cur.row_stride);
    } else {
        REQUIRE(c.bound_io(A.cur) < 0 && A.lag == 0 && c.bound_io(A.out) >= 0);
    }
    // ---- the pointers a launch hands the kernel, from the program: the rows as they are handed in, taps and outputs at their first element,
    // null what is not stored; 16-byte stores of the filtered row where its start and stride are whole vectors
    int out_io = -1, cur_io = -1;
    for (size_t i = fused ? 3 : 2; i < n_ops; ++i) (fused && p.ops[i].src == p.ops[2].dst ? cur_io : out_io) = p.ops[i].io;
    const KernelOnlyArgs launch = launch_args(p, c);
    const ReflectArgs& L = launch.reflect;
    REQUIRE(L.wf == raw_of(p.ops[0].io) && L.taps == first_of(p, p.ops[1].io) && L.out == first_of(p, out_io) && L.cur == first_of(p, cur_io));
    REQUIRE(L.out_vec == vector_store(p, out_io, esz));
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const long programs = argc > 1 ? std::atol(argv[1]) : 20000;
    rng.seed(argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 1);
    long accepted = 0, plain = 0, fused = 0, fused_row = 0, narrow = 0, wide = 0, by_name = 0, shape = 0, too_long = 0, limit = 0;
    for (long number = 0; number < programs; ++number) {
        const Prog p = draw_program();
        const char* why = nullptr;
        const std::unique_ptr<ChainPlan> plan = plan_or_refuse(number, p, &why);
        if (!plan) {
            const bool s = std::strstr(why, "DSP_OP_REFLECTED_CONVOLVE (reflected_convolve_wf) runs on dsp_reflect_kernel only") != nullptr;
            const bool l = std::strstr(why, "The filter is longer than the input waveform") != nullptr;
            const bool x = std::strstr(why, "reflected_convolve_wf: len(w_in) + len(kernel) - 1 of up to") != nullptr;
            shape += s, too_long += l, limit += x;
            if (s || l || x || std::strstr(why, "reflected_convolve_wf") || std::strstr(why, "REFLECTED_CONVOLVE")) ++by_name;
            continue;
        }
        if (!check(number, p, *plan)) return 1;
        if (holds_op(p)) {
            ++accepted;
            ++(plan->only.reflect.wide ? wide : narrow);
            if (plan->only.reflect.lag > 0) {
                ++fused;
                fused_row += plan->bound_io(plan->only.reflect.out) >= 0;
            } else {
                ++plain;
            }
        }
    }
    std::printf("{\"programs\": %ld, \"accepted\": %ld, \"plain\": %ld, \"fused\": %ld, \"fused_row_stored\": %ld, \"narrow\": %ld, \"wide\": %ld, "
                "\"refused_by_name\": %ld, \"refused_shape\": %ld, \"refused_long\": %ld, \"refused_limit\": %ld}\n",
                programs, accepted, plain, fused, fused_row, narrow, wide, by_name, shape, too_long, limit);
    return 0;
}
