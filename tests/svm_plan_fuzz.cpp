// svm_plan_fuzz.cpp -- the planner (dsp_plan.cpp) on programs that hold DSP_OP_SVM_PREDICT, with wild row lengths, support-vector and class
// counts, bindings, offsets and strides: the accepted shape and mutations of it.  A stand-alone program, built with
// -fsanitize=address,undefined (tests/test_svm_plan_fuzz_cpu.py); tests/planner_fuzz.cpp draws the opcodes before this one and stays as it is.
// Every program is planned or refused; a planned one runs on dsp_svm_kernel with an argument block that names bindings of the right kind
// and size and fits the kernel's LDS and accumulators.
//   svm_plan_fuzz <programs> <seed>     prints {"programs": .., "accepted": .., "with_decisions": .., "f64": .., "refused_by_name": ..}
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
    p.dtype = chance(40) ? DSP_F64 : DSP_F32;
    int rows = p.dtype == DSP_F64 ? (chance(50) ? DSP_F64 : DSP_F32) : DSP_F32;
    if (chance(8)) rows = (int)draw(-1, 9);
    int32_t n = clip(wild_length());
    if (chance(75)) n = (int32_t)draw(1, chance(80) ? 300 : 16384);
    int64_t n_sv = chance(80) ? draw(1, chance(80) ? 400 : 70000) : wild_length();
    int32_t k = chance(85) ? (int32_t)draw(2, 23) : clip(wild_length());
    const int64_t pairs = (int64_t)k * (k - 1) / 2;
    const int32_t off = chance(60) ? 0 : (int32_t)(chance(90) ? draw(0, 64) : draw(-4, 0x7fffffff));
    int64_t stride = (int64_t)n + off + (chance(50) ? 0 : draw(0, 40));
    if (chance(8)) stride = chance(50) ? draw(-8, 8) : ((int64_t)1 << draw(31, 62));
    auto taps = [&](int64_t len) {
        const int64_t l = chance(94) ? len : wild_length();
        p.io.push_back({chance(96) ? DSP_IO_TAPS : (int)draw(-1, 5), chance(95) ? DSP_F64 : (int)draw(-1, 9), clip(l), 0, 0});
        return (int)p.io.size() - 1;
    };
    p.slots = {n};
    p.n_sregs = 1;
    p.io.push_back({DSP_IO_WF_IN, rows, n, off, stride});
    p.ops.push_back(make_op(DSP_OP_LOAD, 0, 0, 0));
    const int io_sv = taps(times(n_sv, n)), io_norm = taps(n_sv), io_coef = taps(times(n_sv, pairs)), io_icpt = taps(pairs), io_cls = taps(k);
    int io_dec = -1;
    if (chance(40)) {
        int64_t dec_stride = pairs + (chance(50) ? 0 : draw(0, 9));
        if (chance(8)) dec_stride = chance(50) ? draw(-8, 8) : ((int64_t)1 << draw(31, 62));
        p.io.push_back({chance(95) ? DSP_IO_WF_OUT : (int)draw(-1, 5), chance(92) ? DSP_F64 : (int)draw(-1, 9), clip(chance(92) ? pairs : wild_length()), chance(90) ? 0 : (int32_t)draw(-2, 100), dec_stride});
        io_dec = (int)p.io.size() - 1;
    }
    dsp_op o = make_op(DSP_OP_SVM_PREDICT, 0, 0, io_sv);
    o.ip[0] = io_norm, o.ip[1] = io_coef, o.ip[2] = io_icpt, o.ip[3] = io_cls;
    o.sp[0] = {DSP_ARG_CONST, 0, chance(90) ? 0.01 * (double)draw(1, 400) : (double)draw(-5, 5)};
    o.sp[1] = {DSP_ARG_CONST, 0, chance(92) ? (double)draw(0, 1) : 0.5 * (double)draw(-3, 5)};
    o.sp[2] = {chance(96) ? DSP_ARG_CONST : (int)draw(-1, 3), 0, chance(94) ? (double)io_dec : (chance(50) ? (double)draw(-3, 12) : 0.5 + (double)draw(0, 4))};
    p.ops.push_back(o);
    p.io.push_back({chance(96) ? DSP_IO_SCALAR_OUT : (int)draw(-1, 5), chance(92) ? p.dtype : (int)draw(-1, 9), 1, 0, chance(90) ? 1 : draw(-2, 9)});
    dsp_op st = make_op(DSP_OP_STORE_SCALAR, 0, 0, (int)p.io.size() - 1);
    st.ip[0] = 0;
    p.ops.push_back(st);
    // mutations: a wild field, an op more or less, a slot more, registers
    for (int m = (int)draw(0, 3); m > 0 && chance(45); --m) {
        switch (draw(0, 8)) {
            case 0: p.ops[draw(0, (int64_t)p.ops.size() - 1)].dst = (int32_t)draw(-2, 5); break;
            case 1: p.ops[draw(0, (int64_t)p.ops.size() - 1)].src = (int32_t)draw(-2, 5); break;
            case 2: p.ops[draw(0, (int64_t)p.ops.size() - 1)].io = (int32_t)draw(-2, 9); break;
            case 3: p.ops[draw(0, (int64_t)p.ops.size() - 1)].ip[draw(0, 3)] = (int32_t)(chance(50) ? draw(-3, 9) : draw(-3, 70000)); break;
            case 4: p.ops.erase(p.ops.begin() + draw(0, (int64_t)p.ops.size() - 1)); break;
            case 5: {
                const int extra[] = {DSP_OP_SVM_PREDICT, DSP_OP_NORMALISE, DSP_OP_MIN_MAX, DSP_OP_BL_SUBTRACT, DSP_OP_STORE, DSP_OP_SORT, DSP_OP_LOAD};
                p.ops.insert(p.ops.begin() + draw(0, (int64_t)p.ops.size()), make_op(extra[draw(0, 6)], (int)draw(0, 2), (int)draw(0, 2), (int)draw(0, 3)));
                p.n_sregs = 4;
                break;
            }
            case 6: p.slots.push_back(clip(wild_length())); break;
            case 7: p.n_sregs = (int)draw(-1, 70); break;
            default: p.ops[draw(0, (int64_t)p.ops.size() - 1)].opcode = (int32_t)draw(-1, 60); break;
        }
        if (p.ops.empty()) p.ops.push_back(make_op(DSP_OP_SVM_PREDICT, 0, 0, 0));
    }
    return p;
}

bool holds_svm(const Prog& p) {
    for (const dsp_op& o : p.ops)
        if (o.opcode == DSP_OP_SVM_PREDICT) return true;
    return false;
}

bool check(long number, const Prog& p, const ChainPlan& c) {
    if (!holds_svm(p)) return true;  // (a mutation took the op out: any route, tests/planner_fuzz.cpp's business)
    // (an op of another kernel-only route beside ours belongs to that route, whose shapes hold no SVM_PREDICT: such a program is refused, never accepted)
    REQUIRE(c.kernel_only == DSP_ROUTE_SVM);
    REQUIRE(dsp_plan_route(&c) == DSP_ROUTE_SVM && std::strcmp(dsp_plan_kernel_name(&c), "dsp_svm_kernel") == 0);
    REQUIRE(p.ops.size() == 3 && p.ops[0].opcode == DSP_OP_LOAD && p.ops[1].opcode == DSP_OP_SVM_PREDICT && p.ops[2].opcode == DSP_OP_STORE_SCALAR);
    const dsp_op &op = p.ops[1], &st = p.ops[2];
    const SvmArgs& A = c.only.svm;
    const dsp_io_desc &in = p.io[p.ops[0].io], &out = p.io[st.io];
    REQUIRE(A.len >= 1 && A.len <= DSP_DENSE_N_MAX && A.n_classes >= 2 && A.n_classes <= DSP_SVM_CLASSES_MAX && A.n_sv >= 1);
    REQUIRE(A.n_pairs == A.n_classes * (A.n_classes - 1) / 2 && A.n_pairs <= dsp_svm::P_MAX);
    REQUIRE(A.len == in.len && A.wf_offset == in.offset && A.wf_stride == in.row_stride && in.offset >= 0 && in.row_stride >= (int64_t)in.offset + in.len);
    REQUIRE(A.f64 == (p.dtype == DSP_F64) && out.dtype == p.dtype && out.kind == DSP_IO_SCALAR_OUT && A.label_stride == out.row_stride && (A.linear == 0 || A.linear == 1));
    REQUIRE(in.dtype == DSP_F32 || (in.dtype == DSP_F64 && p.dtype == DSP_F64));
    auto model = [&](int k, int64_t len) { return k >= 0 && k < (int)p.io.size() && p.io[k].kind == DSP_IO_TAPS && p.io[k].dtype == DSP_F64 && p.io[k].len == len; };
    REQUIRE(c.bound_io(A.sv) == op.io && model(c.bound_io(A.sv), (int64_t)A.n_sv * A.len) && c.bound_io(A.sv_norm) == op.ip[0] && model(c.bound_io(A.sv_norm), A.n_sv));
    REQUIRE(c.bound_io(A.coef) == op.ip[1] && model(c.bound_io(A.coef), (int64_t)A.n_sv * A.n_pairs) && c.bound_io(A.intercept) == op.ip[2] && model(c.bound_io(A.intercept), A.n_pairs));
    REQUIRE(c.bound_io(A.classes) == op.ip[3] && model(c.bound_io(A.classes), A.n_classes) && c.bound_io(A.label) == st.io);
    if (c.bound_io(A.dec) >= 0) {
        REQUIRE(c.bound_io(A.dec) < (int)p.io.size());
        const dsp_io_desc& d = p.io[c.bound_io(A.dec)];
        REQUIRE(d.kind == DSP_IO_WF_OUT && d.dtype == DSP_F64 && d.len == A.n_pairs && d.row_stride >= (int64_t)d.offset + d.len && A.dec_stride == d.row_stride);
    } else {
        REQUIRE(c.bound_io(A.dec) == -1);
    }
    REQUIRE(dsp_svm::lds_bytes(A.len, A.n_pairs) <= 149504 && dsp_svm::lds_bytes(A.len, A.n_pairs) <= LDS_BYTES_PER_CU);
    REQUIRE(dsp_svm::pair_blocks(A.n_pairs) <= dsp_svm::built_blocks(A.n_pairs) && dsp_svm::built_blocks(A.n_pairs) <= dsp_svm::PAIR_BLOCKS_MAX);
    REQUIRE(c.only_src.io == p.ops[0].io && c.only_src.dtype == in.dtype);
    // ---- the pointers a launch hands the kernel, from the program: the rows as they are handed in, the model, the label and the decisions at their first element
    const KernelOnlyArgs launch = launch_args(p, c);
    const SvmArgs& L = launch.svm;
    REQUIRE(L.wf == raw_of(p.ops[0].io) && L.sv == first_of(p, op.io) && L.sv_norm == first_of(p, op.ip[0]) && L.coef == first_of(p, op.ip[1]));
    REQUIRE(L.intercept == first_of(p, op.ip[2]) && L.classes == first_of(p, op.ip[3]) && L.label == first_of(p, st.io) && L.dec == first_of(p, (int)op.sp[2].value));
    REQUIRE(!c.only_src.vec || ((in.row_stride * dsp_elem_size(in.dtype)) % 16 == 0 && (in.offset * dsp_elem_size(in.dtype)) % 16 == 0 &&
                               (in.len * dsp_elem_size(in.dtype)) % 16 == 0));
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const long programs = argc > 1 ? std::atol(argv[1]) : 20000;
    rng.seed(argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 1);
    long accepted = 0, with_dec = 0, n_f64 = 0, by_name = 0;
    for (long number = 0; number < programs; ++number) {
        const Prog p = draw_program();
        const char* why = nullptr;
        const std::unique_ptr<ChainPlan> plan = plan_or_refuse(number, p, &why);
        if (!plan) {
            if (std::strstr(why, "runs on dsp_svm_kernel only") || std::strstr(why, "svm_predict: ") || std::strstr(why, "bad SVM_PREDICT")) ++by_name;
            continue;
        }
        if (!check(number, p, *plan)) return 1;
        if (holds_svm(p) && plan->kernel_only == DSP_ROUTE_SVM) {
            ++accepted;
            with_dec += plan->bound_io(plan->only.svm.dec) >= 0;
            n_f64 += plan->f64;
        }
    }
    std::printf("{\"programs\": %ld, \"accepted\": %ld, \"with_decisions\": %ld, \"f64\": %ld, \"refused_by_name\": %ld}\n", programs, accepted, with_dec, n_f64, by_name);
    return 0;
}
