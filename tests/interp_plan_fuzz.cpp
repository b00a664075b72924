// interp_plan_fuzz.cpp -- the planner (dsp_plan.cpp) on programs that hold DSP_OP_INTERP_UPSAMPLE, with wild modes, lengths, slots, offsets
// and strides: the one accepted shape and mutations of it.  A stand-alone program, built with -fsanitize=address,undefined
// (tests/test_interp_index_cpu.py), as tests/sort_plan_fuzz.cpp is for DSP_OP_SORT.  Every program is planned or refused; a planned one runs
// on dsp_interp_kernel with an argument block that names the bindings' geometry, a mode the index rules know and an LDS footprint that fits.
//   interp_plan_fuzz <programs> <seed>     prints {"programs": .., "accepted": .., "narrow": .., "wide": .., "refused_by_name": .., "modes": ..}
#include "plan_fuzz.h"

namespace {

int64_t wild_length() {
    switch (draw(0, 9)) {
        case 0: return draw(-3, 3);
        case 1: return (int64_t)1 << draw(0, 21);
        case 2: return ((int64_t)1 << draw(0, 21)) + draw(-1, 1);
        case 3: return draw(16380, 16390);
        case 4: return chance(50) ? draw(8188, 8196) : draw(5450, 5460);
        case 5: return chance(50) ? draw(2040, 2056) : draw(676, 690);
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
    const int32_t m = chance(30) && n > 0 && n < 100000 ? n * (int32_t)draw(1, 16) : (int32_t)wild_length();
    const char letters[] = "infclhs";
    const int32_t mode = chance(90) ? letters[draw(0, 6)] : (int32_t)draw(-2, 300);
    const int32_t off = chance(60) ? 0 : (int32_t)(chance(90) ? draw(0, 64) : draw(-4, 0x7fffffff));
    int64_t stride = (int64_t)n + off + (chance(50) ? 0 : draw(0, 40));
    if (chance(8)) stride = chance(50) ? draw(-8, 8) : ((int64_t)1 << draw(31, 62));
    int64_t out_stride = (int64_t)m + (chance(50) ? 0 : draw(0, 40));
    if (chance(8)) out_stride = chance(50) ? draw(-8, 8) : ((int64_t)1 << draw(31, 62));
    p.slots = {n, m};
    p.io.push_back({DSP_IO_WF_IN, rows, n, off, stride});
    p.io.push_back({DSP_IO_WF_OUT, chance(92) ? p.dtype : (int)draw(-1, 9), m, chance(90) ? 0 : (int32_t)draw(-2, 100), out_stride});
    p.ops.push_back(make_op(DSP_OP_LOAD, 0, 0, 0));
    p.ops.push_back(make_op(DSP_OP_INTERP_UPSAMPLE, 1, 0, 0));
    p.ops.back().ip[0] = mode;
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
                const int extra[] = {DSP_OP_INTERP_UPSAMPLE, DSP_OP_MIN_MAX, DSP_OP_BL_SUBTRACT, DSP_OP_STORE, DSP_OP_PSD, DSP_OP_COPY, DSP_OP_LOAD};
                p.ops.insert(p.ops.begin() + draw(0, (int64_t)p.ops.size()), make_op(extra[draw(0, 6)], (int)draw(0, 2), (int)draw(0, 2), (int)draw(0, 1)));
                p.n_sregs = 4;
                break;
            }
            case 6: p.slots.push_back((int32_t)wild_length()); break;
            case 7: p.n_sregs = (int)draw(-1, 70); break;
            default: p.ops[draw(0, (int64_t)p.ops.size() - 1)].opcode = (int32_t)draw(-1, 45); break;
        }
        if (p.ops.empty()) p.ops.push_back(make_op(DSP_OP_INTERP_UPSAMPLE, 1, 0, 0));
    }
    return p;
}

bool holds_op(const Prog& p) {
    for (const dsp_op& o : p.ops)
        if (o.opcode == DSP_OP_INTERP_UPSAMPLE) return true;
    return false;
}

bool check(long number, const Prog& p, const ChainPlan& c) {
    if (!holds_op(p)) return true;  // (a mutation took the op out: any route, tests/planner_fuzz.cpp's business)
    REQUIRE(dsp_plan_route(&c) == DSP_ROUTE_INTERP && c.kernel_only == DSP_ROUTE_INTERP);
    REQUIRE(std::strcmp(dsp_plan_kernel_name(&c), "dsp_interp_kernel") == 0);
    REQUIRE(p.ops.size() == 3 && p.ops[0].opcode == DSP_OP_LOAD && p.ops[1].opcode == DSP_OP_INTERP_UPSAMPLE && p.ops[2].opcode == DSP_OP_STORE);
    const InterpArgs& A = c.only.interp;
    const dsp_io_desc &in = p.io[p.ops[0].io], &out = p.io[p.ops[2].io];
    const int esz = p.dtype == DSP_F64 ? 8 : 4;
    REQUIRE(dsp_interp::mode_ok(A.mode) && A.mode == p.ops[1].ip[0]);
    REQUIRE(A.len >= 1 && A.len <= dsp_interp::max_len(A.mode, esz) && A.out_len >= 1);
    REQUIRE(A.mode != 'h' || A.len >= 2);
    REQUIRE(A.mode != 'i' || A.out_len % A.len == 0);
    REQUIRE(A.len == in.len && A.out_len == out.len && A.wf_offset == in.offset && A.wf_stride == in.row_stride && A.out_stride == out.row_stride);
    REQUIRE(in.offset >= 0 && in.row_stride >= (int64_t)in.offset + in.len && out.row_stride >= out.len && out.dtype == p.dtype);
    REQUIRE(A.wide == (dsp_interp::wide(A.mode, A.len, esz) ? 1 : 0));
    REQUIRE(dsp_interp::lds_bytes(A.mode, A.len, esz) <= 64 * 1024 + 16);
    REQUIRE(c.only_src.io == p.ops[0].io && c.only_src.dtype == in.dtype && c.bound_io(A.out) == p.ops[2].io);
    // ---- the pointers a launch hands the kernel, from the program: the rows as they are handed in, the output at its first element, and
    // 16-byte stores where that and the stride are whole vectors
    const KernelOnlyArgs launch = launch_args(p, c);
    REQUIRE(launch.interp.wf == raw_of(p.ops[0].io) && launch.interp.out == first_of(p, p.ops[2].io));
    REQUIRE(launch.interp.out_vec == vector_store(p, p.ops[2].io, p.dtype == DSP_F64 ? 8 : 4));
    REQUIRE(!c.only_src.vec || ((in.row_stride * dsp_elem_size(in.dtype)) % 16 == 0 && (in.offset * dsp_elem_size(in.dtype)) % 16 == 0 &&
                                  (in.len * dsp_elem_size(in.dtype)) % 16 == 0));
    // every output of the planned row has a segment inside the row (a sample of them: the first, the last, and 30 in between)
    for (int k = 0; k <= 31; ++k) {
        const int64_t o = (int64_t)(A.out_len - 1) * k / 31;
        const dsp_interp::Map mp = dsp_interp::map(A.mode, A.len, A.out_len, o);
        REQUIRE(mp.kind == dsp_interp::NONE || (mp.seg >= 0 && mp.seg < A.len));
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const long programs = argc > 1 ? std::atol(argv[1]) : 20000;
    rng.seed(argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 1);
    long accepted = 0, narrow = 0, wide = 0, by_name = 0;
    unsigned modes = 0;
    for (long number = 0; number < programs; ++number) {
        const Prog p = draw_program();
        const char* why = nullptr;
        const std::unique_ptr<ChainPlan> plan = plan_or_refuse(number, p, &why);
        if (!plan) {
            if (std::strstr(why, "DSP_OP_INTERP_UPSAMPLE (interpolating_upsampler) runs on dsp_interp_kernel only") || std::strstr(why, "interpolating_upsampler"))
                ++by_name;
            continue;
        }
        if (!check(number, p, *plan)) return 1;
        if (holds_op(p)) {
            ++accepted;
            ++(plan->only.interp.wide ? wide : narrow);
            modes |= 1u << (std::strchr("infclhs", plan->only.interp.mode) - "infclhs");
        }
    }
    std::printf("{\"programs\": %ld, \"accepted\": %ld, \"narrow\": %ld, \"wide\": %ld, \"refused_by_name\": %ld, \"modes\": %u}\n", programs, accepted, narrow, wide,
                by_name, modes);
    return 0;
}
