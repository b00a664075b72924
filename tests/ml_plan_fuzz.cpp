// ml_plan_fuzz.cpp -- the planner (dsp_plan.cpp) on programs that hold DSP_OP_NORMALISE or DSP_OP_DENSE, with wild lengths, widths, slots,
// bindings, offsets and strides: the three accepted shapes and mutations of them.  A stand-alone program, built with
// -fsanitize=address,undefined (tests/test_ml_plan_fuzz_cpu.py); tests/planner_fuzz.cpp draws the opcodes before these and stays as it is.
// Every program is planned or refused; a planned one runs on dsp_dense_kernel with an argument block that names bindings of the right
// kind and size and fits the kernel's LDS and accumulators.
//   ml_plan_fuzz <programs> <seed>     prints {"programs": .., "accepted": .., "dense": .., "classify": .., "normalise": .., "fused": .., "refused_by_name": ..}
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
        case 4: return draw(250, 260);
        case 5: return draw(60, 70);
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
    if (chance(75)) n = (int32_t)draw(1, chance(80) ? 300 : 16384);
    int32_t m = (int32_t)wild_length();
    if (chance(80)) m = (int32_t)draw(1, 256);
    const bool norm = chance(40), dense = !norm || chance(70), classify = dense && chance(30);
    const bool bias = chance(50);
    const int32_t off = chance(60) ? 0 : (int32_t)(chance(90) ? draw(0, 64) : draw(-4, 0x7fffffff));
    int64_t stride = (int64_t)n + off + (chance(50) ? 0 : draw(0, 40));
    if (chance(8)) stride = chance(50) ? draw(-8, 8) : ((int64_t)1 << draw(31, 62));
    const int32_t out_len = !dense ? n : classify ? 1 : m;
    int64_t out_stride = classify ? 1 : (int64_t)out_len + (chance(50) ? 0 : draw(0, 40));
    if (chance(8)) out_stride = chance(50) ? draw(-8, 8) : ((int64_t)1 << draw(31, 62));
    auto taps = [&](int64_t len) {
        const int64_t l = chance(92) ? len : wild_length();
        p.io.push_back({chance(95) ? DSP_IO_TAPS : (int)draw(-1, 5), chance(95) ? p.dtype : (int)draw(-1, 9), (int32_t)(l > 0x7fffffff ? 0x7fffffff : l), 0, 0});
        return (int)p.io.size() - 1;
    };
    p.slots = {n};
    p.io.push_back({DSP_IO_WF_IN, rows, n, off, stride});
    p.ops.push_back(make_op(DSP_OP_LOAD, 0, 0, 0));
    if (norm) {
        const int im = taps(n), iv = taps(n);
        dsp_op o = make_op(DSP_OP_NORMALISE, 0, 0, im);
        o.ip[0] = iv;
        p.ops.push_back(o);
    }
    if (dense) {
        const int iw = taps((int64_t)n * (classify ? 1 : m)), ib = bias ? taps(classify ? 1 : m) : -1;
        dsp_op o = make_op(DSP_OP_DENSE, classify ? 0 : 1, 0, iw);
        o.ip[0] = (int32_t)(chance(80) ? "srlmt"[draw(0, 4)] : draw(-3, 300));
        o.ip[1] = ib, o.ip[2] = n, o.ip[3] = classify ? 0 : m;
        p.ops.push_back(o);
        if (classify)
            p.n_sregs = 1;
        else
            p.slots.push_back(m);
    }
    p.io.push_back({classify ? DSP_IO_SCALAR_OUT : DSP_IO_WF_OUT, chance(92) ? p.dtype : (int)draw(-1, 9), out_len, chance(90) ? 0 : (int32_t)draw(-2, 100), out_stride});
    const int io_out = (int)p.io.size() - 1;
    if (classify) {
        dsp_op o = make_op(DSP_OP_STORE_SCALAR, 0, 0, io_out);
        o.ip[0] = 0;
        p.ops.push_back(o);
    } else {
        p.ops.push_back(make_op(DSP_OP_STORE, 0, dense ? 1 : 0, io_out));
    }
    // mutations: a wild field, an op more or less, a slot more, registers
    for (int k = (int)draw(0, 3); k > 0 && chance(45); --k) {
        switch (draw(0, 8)) {
            case 0: p.ops[draw(0, (int64_t)p.ops.size() - 1)].dst = (int32_t)draw(-2, 5); break;
            case 1: p.ops[draw(0, (int64_t)p.ops.size() - 1)].src = (int32_t)draw(-2, 5); break;
            case 2: p.ops[draw(0, (int64_t)p.ops.size() - 1)].io = (int32_t)draw(-2, 7); break;
            case 3: p.ops[draw(0, (int64_t)p.ops.size() - 1)].ip[draw(0, 3)] = (int32_t)(chance(50) ? draw(-3, 8) : draw(-3, 70000)); break;
            case 4: p.ops.erase(p.ops.begin() + draw(0, (int64_t)p.ops.size() - 1)); break;
            case 5: {
                const int extra[] = {DSP_OP_DENSE, DSP_OP_NORMALISE, DSP_OP_MIN_MAX, DSP_OP_BL_SUBTRACT, DSP_OP_STORE, DSP_OP_SORT, DSP_OP_LOAD};
                p.ops.insert(p.ops.begin() + draw(0, (int64_t)p.ops.size()), make_op(extra[draw(0, 6)], (int)draw(0, 2), (int)draw(0, 2), (int)draw(0, 3)));
                p.n_sregs = 4;
                break;
            }
            case 6: p.slots.push_back((int32_t)wild_length()); break;
            case 7: p.n_sregs = (int)draw(-1, 70); break;
            default: p.ops[draw(0, (int64_t)p.ops.size() - 1)].opcode = (int32_t)draw(-1, 47); break;
        }
        if (p.ops.empty()) p.ops.push_back(make_op(DSP_OP_DENSE, 1, 0, 0));
    }
    return p;
}

bool holds_layer(const Prog& p) {
    for (const dsp_op& o : p.ops)
        if (o.opcode == DSP_OP_DENSE || o.opcode == DSP_OP_NORMALISE) return true;
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
    if (!holds_layer(p)) return true;  // (a mutation took the ops out: any route, tests/planner_fuzz.cpp's business)
    for (const dsp_op& o : p.ops)      // (an op of another kernel-only route ahead of ours in the table: that route's business)
        if (o.opcode == DSP_OP_SORT) return true;
    REQUIRE(dsp_plan_route(&c) == DSP_ROUTE_DENSE && c.kernel_only == DSP_ROUTE_DENSE);
    REQUIRE(std::strcmp(dsp_plan_kernel_name(&c), "dsp_dense_kernel") == 0);
    const size_t n_ops = p.ops.size();
    REQUIRE(n_ops >= 3 && n_ops <= 4 && p.ops[0].opcode == DSP_OP_LOAD);
    const dsp_op* norm = p.ops[1].opcode == DSP_OP_NORMALISE ? &p.ops[1] : nullptr;
    const dsp_op* dense = p.ops[norm ? 2 : 1].opcode == DSP_OP_DENSE ? &p.ops[norm ? 2 : 1] : nullptr;
    REQUIRE(n_ops == 2u + (norm ? 1 : 0) + (dense ? 1 : 0));
    const dsp_op& st = p.ops[n_ops - 1];
    const bool classify = dense && dense->ip[3] == 0;
    REQUIRE(st.opcode == (classify ? DSP_OP_STORE_SCALAR : DSP_OP_STORE));
    const DenseArgs& A = c.dense;
    const dsp_io_desc &in = p.io[p.ops[0].io], &out = p.io[st.io];
    const int esz = p.dtype == DSP_F64 ? 8 : 4;
    REQUIRE(A.len >= 1 && A.len <= DSP_DENSE_N_MAX && A.m >= 0 && A.m <= DSP_DENSE_M_MAX);
    REQUIRE(A.len == in.len && A.wf_offset == in.offset && A.wf_stride == in.row_stride && A.out_stride == out.row_stride && out.dtype == p.dtype);
    REQUIRE(in.offset >= 0 && in.row_stride >= (int64_t)in.offset + in.len);
    REQUIRE(A.normalise == (norm ? 1 : 0) && (A.m > 0) == (dense != nullptr));
    auto taps_of = [&](int k, int64_t len) { return k >= 0 && k < (int)p.io.size() && p.io[k].kind == DSP_IO_TAPS && p.io[k].dtype == p.dtype && p.io[k].len == len; };
    if (norm) REQUIRE(c.eio_mean == norm->io && c.eio_var == norm->ip[0] && taps_of(c.eio_mean, A.len) && taps_of(c.eio_var, A.len));
    if (dense) {
        REQUIRE(A.m == (classify ? 1 : dense->ip[3]) && A.activation == dense->ip[0] && dense->ip[2] == A.len);
        REQUIRE(c.eio_w == dense->io && taps_of(c.eio_w, (int64_t)A.len * A.m));
        REQUIRE(c.eio_b == dense->ip[1] && (c.eio_b < 0 || taps_of(c.eio_b, A.m)));
        REQUIRE(classify ? out.kind == DSP_IO_SCALAR_OUT : (out.kind == DSP_IO_WF_OUT && out.len == A.m && out.row_stride >= out.len));
        REQUIRE(dsp_dense::lds_bytes(A.m, esz) <= 87040 && dsp_dense::blocks(A.m) <= dsp_dense::built_blocks(A.m));
    } else {
        REQUIRE(c.eio_w < 0 && c.eio_b < 0 && out.kind == DSP_IO_WF_OUT && out.len == A.len && out.row_stride >= out.len);
    }
    REQUIRE(c.dense_src.io == p.ops[0].io && c.dense_src.dtype == in.dtype && c.eio_out == st.io);
    REQUIRE(!c.dense_src.vec || ((in.row_stride * dsp_elem_size(in.dtype)) % 16 == 0 && (in.offset * dsp_elem_size(in.dtype)) % 16 == 0 &&
                                 (in.len * dsp_elem_size(in.dtype)) % 16 == 0));
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const long programs = argc > 1 ? std::atol(argv[1]) : 20000;
    rng.seed(argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 1);
    long accepted = 0, n_dense = 0, n_classify = 0, n_norm = 0, n_fused = 0, by_name = 0;
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
            if (std::strstr(why, "run on dsp_dense_kernel only") || std::strstr(why, "layers of up to") || std::strstr(why, "dense_layer: ") ||
                std::strstr(why, "normalisation_layer: ") || std::strstr(why, "bad DENSE") || std::strstr(why, "bad NORMALISE") || std::strstr(why, "DENSE: ip[2]"))
                ++by_name;
            continue;
        }
        if (!check(number, p, *plan)) return 1;
        if (holds_layer(p) && plan->kernel_only == DSP_ROUTE_DENSE) {
            ++accepted;
            const DenseArgs& A = plan->dense;
            if (A.m == 0)
                ++n_norm;
            else if (p.ops.back().opcode == DSP_OP_STORE_SCALAR)
                ++n_classify;
            else
                ++n_dense;
            if (A.m > 0 && A.normalise) ++n_fused;
        }
    }
    std::printf("{\"programs\": %ld, \"accepted\": %ld, \"dense\": %ld, \"classify\": %ld, \"normalise\": %ld, \"fused\": %ld, \"refused_by_name\": %ld}\n", programs,
                accepted, n_dense, n_classify, n_norm, n_fused, by_name);
    return 0;
}
