// interp_plan_fuzz.cpp -- the planner (dsp_plan.cpp) on programs that hold DSP_OP_INTERP_UPSAMPLE, with wild modes, lengths, slots, offsets
// and strides: the one accepted shape and mutations of it.  A stand-alone program, built with -fsanitize=address,undefined
// (tests/test_interp_index_cpu.py), as tests/sort_plan_fuzz.cpp is for DSP_OP_SORT.  Every program is planned or refused; a planned one runs
// on dsp_interp_kernel with an argument block that names the bindings' geometry, a mode the index rules know and an LDS footprint that fits.
//   interp_plan_fuzz <programs> <seed>     prints {"programs": .., "accepted": .., "narrow": .., "wide": .., "refused_by_name": .., "modes": ..}
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../dspeed_amd/csrc/dsp_plan.h"

namespace {

std::mt19937_64 rng;
int64_t draw(int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); }
bool chance(int percent) { return draw(0, 99) < percent; }

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

struct Prog {
    std::vector<dsp_op> ops;
    std::vector<dsp_io_desc> io;
    std::vector<int32_t> slots;
    int n_sregs = 0, dtype = DSP_F32;
};

dsp_op make_op(int opcode, int dst, int src, int io) {
    dsp_op o;
    std::memset(&o, 0, sizeof o);
    o.opcode = opcode, o.dst = dst, o.src = src, o.io = io;
    return o;
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

#define REQUIRE(cond)                                                          \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("program %ld: accepted, but not %s\n", number, #cond); \
            return false;                                                      \
        }                                                                      \
    } while (0)

bool check(long number, const Prog& p, const ChainPlan& c) {
    if (!holds_op(p)) return true;  // (a mutation took the op out: any route, tests/planner_fuzz.cpp's business)
    REQUIRE(dsp_plan_route(&c) == DSP_ROUTE_INTERP && c.kernel_only == DSP_ROUTE_INTERP);
    REQUIRE(std::strcmp(dsp_plan_kernel_name(&c), "dsp_interp_kernel") == 0);
    REQUIRE(p.ops.size() == 3 && p.ops[0].opcode == DSP_OP_LOAD && p.ops[1].opcode == DSP_OP_INTERP_UPSAMPLE && p.ops[2].opcode == DSP_OP_STORE);
    const InterpArgs& A = c.interp;
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
    REQUIRE(c.interp_src.io == p.ops[0].io && c.interp_src.dtype == in.dtype && c.iuo_out == p.ops[2].io);
    REQUIRE(!c.interp_src.vec || ((in.row_stride * dsp_elem_size(in.dtype)) % 16 == 0 && (in.offset * dsp_elem_size(in.dtype)) % 16 == 0 &&
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
        std::unique_ptr<ChainPlan> plan(new ChainPlan());
        const int rc = dsp_plan_build(plan.get(), p.ops.data(), (int)p.ops.size(), p.io.data(), (int)p.io.size(), p.slots.data(), (int)p.slots.size(),
                                      p.n_sregs, p.dtype);
        if (rc != DSP_OK) {
            const char* why = dsp_plan_last_error();
            if (!why || !*why) {
                std::printf("program %ld: refused (%d) without a reason\n", number, rc);
                return 1;
            }
            if (std::strstr(why, "DSP_OP_INTERP_UPSAMPLE (interpolating_upsampler) runs on dsp_interp_kernel only") || std::strstr(why, "interpolating_upsampler"))
                ++by_name;
            continue;
        }
        if (!check(number, p, *plan)) return 1;
        if (holds_op(p)) {
            ++accepted;
            ++(plan->interp.wide ? wide : narrow);
            modes |= 1u << (std::strchr("infclhs", plan->interp.mode) - "infclhs");
        }
    }
    std::printf("{\"programs\": %ld, \"accepted\": %ld, \"narrow\": %ld, \"wide\": %ld, \"refused_by_name\": %ld, \"modes\": %u}\n", programs, accepted, narrow, wide,
                by_name, modes);
    return 0;
}
