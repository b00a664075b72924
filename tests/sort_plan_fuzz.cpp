// sort_plan_fuzz.cpp -- the planner (dsp_plan.cpp) on programs that hold DSP_OP_SORT, with wild lengths, slots, offsets and strides: the
// one accepted shape and mutations of it.  A stand-alone program, built with -fsanitize=address,undefined (tests/test_sort_network_cpu.py);
// tests/planner_fuzz.cpp draws the opcodes before this one and stays as it is.  Every program is planned or refused; a planned one runs on
// dsp_sort_kernel with an argument block that names the bindings' geometry and fits the kernel's LDS.
//   sort_plan_fuzz <programs> <seed>     prints {"programs": .., "accepted": .., "narrow": .., "wide": .., "refused_by_name": ..}
#include "plan_fuzz.h"

namespace {

int64_t wild_length() {
    switch (draw(0, 9)) {
        case 0: return draw(-3, 3);
        case 1: return (int64_t)1 << draw(0, 21);
        case 2: return ((int64_t)1 << draw(0, 21)) + draw(-1, 1);
        case 3: return draw(16380, 16390);
        case 4: return draw(8188, 8196);
        case 5: return draw(2040, 2056);
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
    int32_t n = (int32_t)wild_length();
    if (chance(70)) n = (int32_t)draw(1, p.dtype == DSP_F64 ? 8192 : 16384);
    const int32_t m = chance(90) ? n : (int32_t)wild_length();
    const int32_t off = chance(60) ? 0 : (int32_t)(chance(90) ? draw(0, 64) : draw(-4, 0x7fffffff));
    int64_t stride = (int64_t)n + off + (chance(50) ? 0 : draw(0, 40));
    if (chance(8)) stride = chance(50) ? draw(-8, 8) : ((int64_t)1 << draw(31, 62));
    int64_t out_stride = (int64_t)m + (chance(50) ? 0 : draw(0, 40));
    if (chance(8)) out_stride = chance(50) ? draw(-8, 8) : ((int64_t)1 << draw(31, 62));
    p.slots = {n, m};
    p.io.push_back({DSP_IO_WF_IN, rows, n, off, stride});
    p.io.push_back({DSP_IO_WF_OUT, chance(92) ? p.dtype : (int)draw(-1, 9), m, chance(90) ? 0 : (int32_t)draw(-2, 100), out_stride});
    p.ops.push_back(make_op(DSP_OP_LOAD, 0, 0, 0));
    p.ops.push_back(make_op(DSP_OP_SORT, 1, 0, 0));
    p.ops.push_back(make_op(DSP_OP_STORE, 0, 1, 1));
    // mutations: a wild field, an op more or less, a slot more, registers
    for (int k = (int)draw(0, 3); k > 0 && chance(45); --k) {
        switch (draw(0, 8)) {
            case 0: p.ops[draw(0, (int64_t)p.ops.size() - 1)].dst = (int32_t)draw(-2, 5); break;
            case 1: p.ops[draw(0, (int64_t)p.ops.size() - 1)].src = (int32_t)draw(-2, 5); break;
            case 2: p.ops[draw(0, (int64_t)p.ops.size() - 1)].io = (int32_t)draw(-2, 4); break;
            case 3: p.ops[draw(0, (int64_t)p.ops.size() - 1)].ip[draw(0, 3)] = (int32_t)draw(-3, 70000); break;
            case 4: p.ops.erase(p.ops.begin() + draw(0, (int64_t)p.ops.size() - 1)); break;
            case 5: {
                const int extra[] = {DSP_OP_SORT, DSP_OP_MIN_MAX, DSP_OP_BL_SUBTRACT, DSP_OP_STORE, DSP_OP_PSD, DSP_OP_COPY, DSP_OP_LOAD};
                p.ops.insert(p.ops.begin() + draw(0, (int64_t)p.ops.size()), make_op(extra[draw(0, 6)], (int)draw(0, 2), (int)draw(0, 2), (int)draw(0, 1)));
                p.n_sregs = 4;
                break;
            }
            case 6: p.slots.push_back((int32_t)wild_length()); break;
            case 7: p.n_sregs = (int)draw(-1, 70); break;
            default: p.ops[draw(0, (int64_t)p.ops.size() - 1)].opcode = (int32_t)draw(-1, 45); break;
        }
        if (p.ops.empty()) p.ops.push_back(make_op(DSP_OP_SORT, 1, 0, 0));
    }
    return p;
}

bool holds_sort(const Prog& p) {
    for (const dsp_op& o : p.ops)
        if (o.opcode == DSP_OP_SORT) return true;
    return false;
}

bool check(long number, const Prog& p, const ChainPlan& c) {
    if (!holds_sort(p)) return true;  // (a mutation took the op out: any route, tests/planner_fuzz.cpp's business)
    REQUIRE(dsp_plan_route(&c) == DSP_ROUTE_SORT && c.kernel_only == DSP_ROUTE_SORT);
    REQUIRE(std::strcmp(dsp_plan_kernel_name(&c), "dsp_sort_kernel") == 0);
    REQUIRE(p.ops.size() == 3 && p.ops[0].opcode == DSP_OP_LOAD && p.ops[1].opcode == DSP_OP_SORT && p.ops[2].opcode == DSP_OP_STORE);
    const SortArgs& A = c.only.sort;
    const dsp_io_desc &in = p.io[p.ops[0].io], &out = p.io[p.ops[2].io];
    const int esz = p.dtype == DSP_F64 ? 8 : 4;
    REQUIRE(A.len >= 1 && A.len <= DSP_SORT_F32_MAX / (esz / 4));
    REQUIRE(A.len == in.len && A.len == out.len && A.wf_offset == in.offset && A.wf_stride == in.row_stride && A.out_stride == out.row_stride);
    REQUIRE(in.offset >= 0 && in.row_stride >= (int64_t)in.offset + in.len && out.row_stride >= out.len && out.dtype == p.dtype);
    REQUIRE(A.padded == dsp_sort::padded(A.len) && A.padded >= A.len && A.wide == (dsp_sort::wide(A.len) ? 1 : 0));
    REQUIRE(dsp_sort::lds_bytes(A.len, esz) <= 64 * 1024 + 16);
    REQUIRE(c.only_src.io == p.ops[0].io && c.only_src.dtype == in.dtype && c.bound_io(A.out) == p.ops[2].io);
    // ---- the pointers a launch hands the kernel, from the program: the rows as they are handed in, the output at its first element
    const KernelOnlyArgs launch = launch_args(p, c);
    REQUIRE(launch.sort.wf == raw_of(p.ops[0].io) && launch.sort.out == first_of(p, p.ops[2].io));
    REQUIRE(!c.only_src.vec || ((in.row_stride * dsp_elem_size(in.dtype)) % 16 == 0 && (in.offset * dsp_elem_size(in.dtype)) % 16 == 0 &&
                                (in.len * dsp_elem_size(in.dtype)) % 16 == 0));
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const long programs = argc > 1 ? std::atol(argv[1]) : 20000;
    rng.seed(argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 1);
    long accepted = 0, narrow = 0, wide = 0, by_name = 0;
    for (long number = 0; number < programs; ++number) {
        const Prog p = draw_program();
        const char* why = nullptr;
        const std::unique_ptr<ChainPlan> plan = plan_or_refuse(number, p, &why);
        if (!plan) {
            if (std::strstr(why, "DSP_OP_SORT (sort) runs on dsp_sort_kernel only") || std::strstr(why, "sort: rows of up to")) ++by_name;
            continue;
        }
        if (!check(number, p, *plan)) return 1;
        if (holds_sort(p)) {
            ++accepted;
            ++(plan->only.sort.wide ? wide : narrow);
        }
    }
    std::printf("{\"programs\": %ld, \"accepted\": %ld, \"narrow\": %ld, \"wide\": %ld, \"refused_by_name\": %ld}\n", programs, accepted, narrow, wide, by_name);
    return 0;
}
