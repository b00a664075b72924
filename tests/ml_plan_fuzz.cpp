// ml_plan_fuzz.cpp -- the planner (dsp_plan.cpp) on programs that hold DSP_OP_NORMALISE or DSP_OP_DENSE, with wild lengths, widths, slots,
// bindings, offsets and strides: the three accepted shapes and mutations of them.  A stand-alone program, built with
// -fsanitize=address,undefined (tests/test_ml_plan_fuzz_cpu.py); tests/planner_fuzz.cpp draws the opcodes before these and stays as it is.
// Every program is planned or refused; a planned one runs on dsp_dense_kernel with an argument block that names bindings of the right
// kind and size and fits the kernel's LDS and accumulators.
//   ml_plan_fuzz <programs> <seed>     prints {"programs": .., "accepted": .., "dense": .., "classify": .., "normalise": .., "fused": .., "refused_by_name": ..}
#include "plan_fuzz.h"

namespace {

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
    const DenseArgs& A = c.only.dense;
    const dsp_io_desc &in = p.io[p.ops[0].io], &out = p.io[st.io];
    const int esz = p.dtype == DSP_F64 ? 8 : 4;
    REQUIRE(A.len >= 1 && A.len <= DSP_DENSE_N_MAX && A.m >= 0 && A.m <= DSP_DENSE_M_MAX);
    REQUIRE(A.len == in.len && A.wf_offset == in.offset && A.wf_stride == in.row_stride && A.out_stride == out.row_stride && out.dtype == p.dtype);
    REQUIRE(in.offset >= 0 && in.row_stride >= (int64_t)in.offset + in.len);
    REQUIRE(A.normalise == (norm ? 1 : 0) && (A.m > 0) == (dense != nullptr));
    auto taps_of = [&](int k, int64_t len) { return k >= 0 && k < (int)p.io.size() && p.io[k].kind == DSP_IO_TAPS && p.io[k].dtype == p.dtype && p.io[k].len == len; };
    if (norm) REQUIRE(c.bound_io(A.means) == norm->io && c.bound_io(A.variances) == norm->ip[0] && taps_of(c.bound_io(A.means), A.len) && taps_of(c.bound_io(A.variances), A.len));
    if (dense) {
        REQUIRE(A.m == (classify ? 1 : dense->ip[3]) && A.activation == dense->ip[0] && dense->ip[2] == A.len);
        REQUIRE(c.bound_io(A.weights) == dense->io && taps_of(c.bound_io(A.weights), (int64_t)A.len * A.m));
        REQUIRE(c.bound_io(A.bias) == dense->ip[1] && (c.bound_io(A.bias) < 0 || taps_of(c.bound_io(A.bias), A.m)));
        REQUIRE(classify ? out.kind == DSP_IO_SCALAR_OUT : (out.kind == DSP_IO_WF_OUT && out.len == A.m && out.row_stride >= out.len));
        REQUIRE(dsp_dense::lds_bytes(A.m, esz) <= 87040 && dsp_dense::blocks(A.m) <= dsp_dense::built_blocks(A.m));
    } else {
        REQUIRE(c.bound_io(A.weights) < 0 && c.bound_io(A.bias) < 0 && out.kind == DSP_IO_WF_OUT && out.len == A.len && out.row_stride >= out.len);
    }
    REQUIRE(c.only_src.io == p.ops[0].io && c.only_src.dtype == in.dtype && c.bound_io(A.out) == st.io);
    REQUIRE(!c.only_src.vec || ((in.row_stride * dsp_elem_size(in.dtype)) % 16 == 0 && (in.offset * dsp_elem_size(in.dtype)) % 16 == 0 &&
                                 (in.len * dsp_elem_size(in.dtype)) % 16 == 0));
    // ---- the pointers a launch hands the kernel, from the program: the rows as they are handed in, every other at its first element, null what the program has not
    const KernelOnlyArgs launch = launch_args(p, c);
    const DenseArgs& L = launch.dense;
    REQUIRE(L.wf == raw_of(p.ops[0].io) && L.out == first_of(p, st.io));
    REQUIRE(L.means == first_of(p, norm ? norm->io : -1) && L.variances == first_of(p, norm ? norm->ip[0] : -1));
    REQUIRE(L.weights == first_of(p, dense ? dense->io : -1) && L.bias == first_of(p, dense ? dense->ip[1] : -1));
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const long programs = argc > 1 ? std::atol(argv[1]) : 20000;
    rng.seed(argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 1);
    long accepted = 0, n_dense = 0, n_classify = 0, n_norm = 0, n_fused = 0, by_name = 0;
    for (long number = 0; number < programs; ++number) {
        const Prog p = draw_program();
        const char* why = nullptr;
        const std::unique_ptr<ChainPlan> plan = plan_or_refuse(number, p, &why);
        if (!plan) {
            if (std::strstr(why, "run on dsp_dense_kernel only") || std::strstr(why, "layers of up to") || std::strstr(why, "dense_layer: ") ||
                std::strstr(why, "normalisation_layer: ") || std::strstr(why, "bad DENSE") || std::strstr(why, "bad NORMALISE") || std::strstr(why, "DENSE: ip[2]"))
                ++by_name;
            continue;
        }
        if (!check(number, p, *plan)) return 1;
        if (holds_layer(p) && plan->kernel_only == DSP_ROUTE_DENSE) {
            ++accepted;
            const DenseArgs& A = plan->only.dense;
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
