// align_plan_fuzz.cpp -- the planner (dsp_plan.cpp) on programs that hold DSP_OP_INL_CORRECTION, DSP_OP_WF_CENTROID, DSP_OP_WF_ALIGNMENT and
// DSP_OP_WF_CORRECTION, with wild lengths, sizes, indices, slots, bindings, offsets and strides: the five accepted shapes (each processor alone,
// wf_alignment -> wf_correction with the aligned row stored or not) and mutations of them.  A stand-alone program, built with
// -fsanitize=address,undefined (tests/test_align_plan_fuzz_cpu.py), as tests/tailfit_plan_fuzz.cpp is for the decay-tail fitter's ops.  Every
// program is planned or refused; a planned one has one of the five shapes and runs on dsp_align_kernel with an argument block whose lengths,
// indices and bindings are in range -- what the kernel forms its addresses from.
//   align_plan_fuzz <programs> <seed>     prints {"programs": .., "accepted": .., "inl": .., "centroid": .., "align": .., "correct": .., "fused": ..,
//                                                  "aligned_stored": .., "per_event": .., "integer_rows": .., "refused_by_name": .., "refused_shape": ..,
//                                                  "refused_check": ..}
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

double wild_number(int32_t n) {
    switch (draw(0, 9)) {
        case 0: return std::numeric_limits<double>::quiet_NaN();
        case 1: return chance(50) ? std::numeric_limits<double>::infinity() : -std::numeric_limits<double>::infinity();
        case 2: return (double)draw(-5, 5);
        case 3: return (double)n + (double)draw(-2, 2);
        case 4: return (double)draw(0, 2 * (int64_t)(n > 0 ? n : 1)) / 2.0;
        case 5: return 1e300;
        default: return (double)draw(0, n > 0 ? n : 1);
    }
}

Prog draw_program() {
    Prog p;
    p.dtype = chance(35) ? DSP_F64 : DSP_F32;
    // 0: inl_correction, 1: get_wf_centroid, 2: wf_alignment, 3: wf_correction, 4: wf_alignment -> wf_correction
    const int kind = (int)draw(0, 4);
    const int ints[] = {DSP_I16, DSP_U16, DSP_I32, DSP_U32};
    int rows = p.dtype == DSP_F64 ? DSP_F64 : DSP_F32;
    if (kind == 0 || ((kind == 2 || kind == 4) && chance(50))) rows = ints[draw(0, 3)];
    else if (p.dtype == DSP_F32 && chance(30)) rows = ints[draw(0, 1)];
    if (chance(6)) rows = (int)draw(-1, 9);
    int32_t n = (int32_t)wild_length();
    if (chance(70)) n = (int32_t)draw(1, 9000);
    const int32_t size = chance(85) ? (int32_t)draw(1, n > 0 ? n : 1) : (int32_t)wild_length();
    const int32_t out_len = kind == 2 || kind == 4 ? (chance(92) ? size : (int32_t)wild_length()) : (chance(92) ? n : (int32_t)wild_length());
    const int32_t off = chance(60) ? 0 : (int32_t)(chance(90) ? draw(0, 64) : draw(-4, 0x7fffffff));
    int64_t stride = (int64_t)n + off + (chance(50) ? 0 : draw(0, 40));
    if (chance(8)) stride = chance(50) ? draw(-8, 8) : ((int64_t)1 << draw(31, 62));
    int64_t out_stride = (int64_t)out_len + (chance(50) ? 0 : draw(0, 40));
    if (chance(8)) out_stride = chance(50) ? draw(-8, 8) : ((int64_t)1 << draw(31, 62));
    auto table = [&](int32_t len) {
        p.io.push_back({chance(95) ? DSP_IO_TAPS : (int)draw(0, 5), chance(92) ? p.dtype : (int)draw(-1, 9), len, 0, 0});
        return (int)p.io.size() - 1;
    };
    auto store = [&](int slot, int32_t len) {
        p.io.push_back({DSP_IO_WF_OUT, chance(92) ? p.dtype : (int)draw(-1, 9), len, chance(90) ? 0 : (int32_t)draw(-2, 100), out_stride});
        p.ops.push_back(make_op(DSP_OP_STORE, 0, slot, (int)p.io.size() - 1));
    };
    auto indices = [&](dsp_op& o, int32_t len, int32_t m) {
        int32_t start = (int32_t)draw(0, len > 1 ? len - 1 : 0);
        const int64_t end = (int64_t)start + draw(1, m > 0 ? m : 1);
        int32_t stop = (int32_t)(end > len ? len : end);
        if (chance(15)) start = (int32_t)draw(-3, (int64_t)len + 3);
        if (chance(15)) stop = (int32_t)(chance(50) ? draw(-3, (int64_t)len + 3) : wild_length());
        o.ip[0] = start, o.ip[1] = stop;
    };
    p.slots = {n};
    p.io.push_back({DSP_IO_WF_IN, rows, n, off, stride});  // 0
    p.ops.push_back(make_op(DSP_OP_LOAD, 0, 0, 0));
    if (kind == 0) {
        p.slots.push_back(out_len);
        p.ops.push_back(make_op(DSP_OP_INL_CORRECTION, 1, 0, table(chance(90) ? (int32_t)draw(1, 70000) : (int32_t)wild_length())));
        store(1, out_len);
    } else if (kind == 1) {
        p.n_sregs = chance(95) ? 1 : (int)draw(-1, 3);
        dsp_op o = make_op(DSP_OP_WF_CENTROID, chance(95) ? 0 : (int)draw(-2, 3), 0, 0);
        o.sp[0] = {DSP_ARG_CONST, 0, chance(80) ? (double)draw(0, n > 1 ? n - 1 : 0) : wild_number(n)};
        if (chance(5)) o.sp[0].kind = (int)draw(0, 3);
        p.ops.push_back(o);
        p.io.push_back({DSP_IO_SCALAR_OUT, chance(92) ? p.dtype : (int)draw(-1, 9), 1, 0, 1});
        p.ops.push_back(make_op(DSP_OP_STORE_SCALAR, 0, 0, (int)p.io.size() - 1));
        p.ops.back().ip[0] = chance(95) ? 0 : (int32_t)draw(-1, 3);
    } else if (kind == 2 || kind == 4) {
        p.slots.push_back(out_len);
        dsp_op o = make_op(DSP_OP_WF_ALIGNMENT, 1, 0, 0);
        o.sp[0] = {DSP_ARG_CONST, 0, chance(85) ? (double)draw(-20, (int64_t)n + 20) / 2.0 : wild_number(n)};
        if (chance(45)) {
            p.io.push_back({chance(95) ? DSP_IO_SCALAR_IN : (int)draw(0, 5), chance(92) ? p.dtype : (int)draw(-1, 9), 1, 0, chance(90) ? 1 : draw(0, 3)});
            o.sp[0].kind = chance(95) ? DSP_ARG_INPUT : (int)draw(0, 3);
            o.sp[0].index = (int32_t)p.io.size() - 1;
        }
        o.sp[1] = {DSP_ARG_CONST, 0, chance(85) ? (double)draw(0, n > 0 ? n : 0) : wild_number(n)};
        o.sp[2] = {DSP_ARG_CONST, 0, chance(90) ? (double)size : wild_number(n)};
        for (int k = 1; k < 3; ++k)
            if (chance(3)) o.sp[k].kind = (int)draw(0, 3);
        p.ops.push_back(o);
        if (kind == 4) {
            p.slots.push_back(chance(95) ? out_len : (int32_t)wild_length());
            const int32_t m = chance(90) ? (int32_t)draw(1, 300) : (int32_t)wild_length();
            dsp_op c = make_op(DSP_OP_WF_CORRECTION, 2, 1, table(m));
            indices(c, out_len, m);
            p.ops.push_back(c);
            if (chance(50)) store(1, out_len);
            store(2, p.slots[2]);
        } else {
            store(1, out_len);
        }
    } else {
        p.slots.push_back(out_len);
        const int32_t m = chance(90) ? (int32_t)draw(1, 300) : (int32_t)wild_length();
        dsp_op c = make_op(DSP_OP_WF_CORRECTION, 1, 0, table(m));
        indices(c, n, m);
        p.ops.push_back(c);
        store(1, out_len);
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
                const int extra[] = {DSP_OP_INL_CORRECTION, DSP_OP_WF_CENTROID, DSP_OP_WF_ALIGNMENT, DSP_OP_WF_CORRECTION, DSP_OP_MIN_MAX, DSP_OP_BL_SUBTRACT, DSP_OP_STORE, DSP_OP_LOAD};
                p.ops.insert(p.ops.begin() + draw(0, (int64_t)p.ops.size()), make_op(extra[draw(0, 7)], (int)draw(0, 3), (int)draw(0, 3), (int)draw(0, 3)));
                p.n_sregs = 4;
                break;
            }
            case 6: p.slots.push_back((int32_t)wild_length()); break;
            case 7: p.n_sregs = (int)draw(-1, 70); break;
            default: p.ops[draw(0, (int64_t)p.ops.size() - 1)].opcode = (int32_t)draw(-1, 58); break;
        }
        if (p.ops.empty()) p.ops.push_back(make_op(DSP_OP_WF_CENTROID, 0, 0, 0));
    }
    return p;
}

bool is_mine(int opcode) { return opcode >= DSP_OP_INL_CORRECTION && opcode <= DSP_OP_WF_CORRECTION; }
bool holds_op(const Prog& p) {
    for (const dsp_op& o : p.ops)
        if (is_mine(o.opcode)) return true;
    return false;
}
bool integer_rows(int dtype) { return dtype == DSP_I16 || dtype == DSP_U16 || dtype == DSP_I32 || dtype == DSP_U32; }

bool check(long number, const Prog& p, const ChainPlan& c) {
    if (!holds_op(p)) return true;  // (a mutation took the ops out: any route, tests/planner_fuzz.cpp's business)
    if (c.kernel_only != DSP_ROUTE_ALIGN) {
        std::printf("program %ld: holds the op and is planned on route %d\n", number, (int)c.kernel_only);
        return false;
    }
    REQUIRE(dsp_plan_route(&c) == DSP_ROUTE_ALIGN);
    REQUIRE(std::strcmp(dsp_plan_kernel_name(&c), "dsp_align_kernel") == 0);
    const AlignArgs& A = c.only.align;
    const size_t n_ops = p.ops.size();
    // ---- one of the five shapes, and nothing else
    REQUIRE(n_ops >= 3 && n_ops <= 5 && p.ops[0].opcode == DSP_OP_LOAD);
    const int first = p.ops[1].opcode;
    const bool fused = first == DSP_OP_WF_ALIGNMENT && p.ops[2].opcode == DSP_OP_WF_CORRECTION;
    REQUIRE(is_mine(first) && A.mode == first - DSP_OP_INL_CORRECTION + 1 && A.correct == (fused ? 1 : 0));
    REQUIRE(n_ops == (size_t)(fused ? (c.bound_io(A.out) >= 0 ? 5 : 4) : 3));
    for (size_t i = fused ? 3 : 2; i < n_ops; ++i) REQUIRE(p.ops[i].opcode == (first == DSP_OP_WF_CENTROID ? DSP_OP_STORE_SCALAR : DSP_OP_STORE));
    REQUIRE((int)p.slots.size() == (first == DSP_OP_WF_CENTROID ? 1 : (fused ? 3 : 2)));
    REQUIRE(A.f64 == (p.dtype == DSP_F64 ? 1 : 0));
    // ---- the rows
    const dsp_io_desc& in = p.io[c.only_src.io];
    REQUIRE(in.kind == DSP_IO_WF_IN && A.len >= 1 && A.len == in.len && A.len == p.slots[0] && A.wf_offset == in.offset && A.wf_stride == in.row_stride);
    REQUIRE(in.offset >= 0 && in.row_stride >= (int64_t)in.offset + in.len && c.only_src.dtype == in.dtype);
    REQUIRE(!c.only_src.vec || ((in.row_stride * dsp_elem_size(in.dtype)) % 16 == 0 && (in.offset * dsp_elem_size(in.dtype)) % 16 == 0 &&
                                 (in.len * dsp_elem_size(in.dtype)) % 16 == 0));
    const bool loop_rows = p.dtype == DSP_F64 ? in.dtype == DSP_F64 : (in.dtype == DSP_F32 || in.dtype == DSP_I16 || in.dtype == DSP_U16);
    if (A.mode == DSP_ALIGN_INL) REQUIRE(integer_rows(in.dtype));
    else if (A.mode == DSP_ALIGN_WINDOW) REQUIRE(in.dtype == p.dtype || in.dtype == DSP_I16 || in.dtype == DSP_U16 || (p.dtype == DSP_F64 && integer_rows(in.dtype)));
    else REQUIRE(loop_rows);
    // ---- the parameters: what the kernel forms addresses from
    const bool has_table = A.mode == DSP_ALIGN_INL || A.mode == DSP_ALIGN_CORRECT || fused;
    if (has_table) {
        REQUIRE(c.bound_io(A.table) >= 0 && c.bound_io(A.table) < (int)p.io.size());
        const dsp_io_desc& t = p.io[c.bound_io(A.table)];
        REQUIRE(t.kind == DSP_IO_TAPS && t.dtype == p.dtype && t.len >= 1 && A.table_len == t.len);
    } else {
        REQUIRE(c.bound_io(A.table) < 0);
    }
    if (A.mode == DSP_ALIGN_CENTROID) {
        REQUIRE(A.shift >= 0 && A.shift <= A.len - 1 && c.bound_io(A.scalar_out) >= 0 && p.io[c.bound_io(A.scalar_out)].kind == DSP_IO_SCALAR_OUT && p.io[c.bound_io(A.scalar_out)].dtype == p.dtype);
        REQUIRE(c.bound_io(A.out) < 0 && c.bound_io(A.out2) < 0 && c.bound_io(A.centroid) < 0);
    } else {
        REQUIRE(c.bound_io(A.scalar_out) < 0);
    }
    if (A.mode == DSP_ALIGN_WINDOW) {
        REQUIRE(A.size >= 1 && A.size <= A.len && A.size == p.slots[1] && A.shift >= 0 && A.shift <= A.len);
        if (c.bound_io(A.centroid) >= 0) REQUIRE(p.io[c.bound_io(A.centroid)].kind == DSP_IO_SCALAR_IN && p.io[c.bound_io(A.centroid)].dtype == p.dtype && A.centroid_stride == p.io[c.bound_io(A.centroid)].row_stride);
        else REQUIRE(A.centroid_const == A.centroid_const);  // (a NaN constant is refused at the plan)
        const AlignWindow w = dsp_align_window(c.bound_io(A.centroid) >= 0 ? 3.5 : A.centroid_const, A.shift, A.size, A.len);
        REQUIRE(w.kind >= 0 && w.kind <= 3 && (w.kind != 1 || (w.first >= 0 && w.first + A.size <= A.len)) &&
                (w.kind != 2 || (w.fill >= 0 && w.fill <= A.size && w.count >= 0 && w.count <= A.len && (w.count == 1 || w.fill + w.count == A.size))));
    }
    if (A.mode == DSP_ALIGN_CORRECT || fused) {
        const int rows_len = fused ? A.size : A.len;
        REQUIRE(A.start >= 0 && A.start < A.stop && A.stop <= rows_len && A.stop - A.start <= A.table_len);
    }
    // ---- the outputs
    const int out_len = A.mode == DSP_ALIGN_WINDOW ? A.size : A.len;
    if (A.mode != DSP_ALIGN_CENTROID) {
        const int last = fused ? c.bound_io(A.out2) : c.bound_io(A.out);
        REQUIRE(last >= 0 && (fused || c.bound_io(A.out2) < 0));
        for (int k : {c.bound_io(A.out), c.bound_io(A.out2)}) {
            if (k < 0) continue;
            const dsp_io_desc& o = p.io[k];
            REQUIRE(o.kind == DSP_IO_WF_OUT && o.dtype == p.dtype && o.len == out_len && o.offset >= 0 && o.row_stride >= (int64_t)o.offset + o.len);
            REQUIRE((k == c.bound_io(A.out) ? A.out_stride : A.out2_stride) == o.row_stride);
        }
        REQUIRE(c.bound_io(A.out) != c.bound_io(A.out2));
    }
    // ---- the pointers a launch hands the kernel, from the program: the rows as they are handed in, table, column and outputs at their first
    // element, null what the program has not; 16-byte stores of the rows the kernel streams out (not the aligned row's) where their start and
    // stride are whole vectors.  table_nan is the chain's own: not filled here
    const dsp_op& with_table = fused ? p.ops[2] : p.ops[1];
    int out_io = -1, out2_io = -1;
    if (first != DSP_OP_WF_CENTROID)
        for (size_t i = fused ? 3 : 2; i < n_ops; ++i) (fused && p.ops[i].src == p.ops[2].dst ? out2_io : out_io) = p.ops[i].io;
    const KernelOnlyArgs launch = launch_args(p, c);
    const AlignArgs& L = launch.align;
    REQUIRE(L.wf == raw_of(p.ops[0].io) && L.table == first_of(p, has_table ? with_table.io : -1) && L.table_nan == nullptr);
    REQUIRE(L.centroid == first_of(p, first == DSP_OP_WF_ALIGNMENT ? column_of(p.ops[1], 0) : -1) && L.scalar_out == first_of(p, first == DSP_OP_WF_CENTROID ? p.ops[2].io : -1));
    REQUIRE(L.out == first_of(p, out_io) && L.out2 == first_of(p, out2_io));
    REQUIRE(L.out_vec == (first == DSP_OP_WF_ALIGNMENT ? 0 : vector_store(p, out_io, p.dtype == DSP_F64 ? 8 : 4)));
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const long programs = argc > 1 ? std::atol(argv[1]) : 20000;
    rng.seed(argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 1);
    long accepted = 0, kinds[5] = {0, 0, 0, 0, 0}, aligned_stored = 0, per_event = 0, ints = 0, by_name = 0, shape = 0, checks = 0;
    // the windows of every centroid, shift and size a row can meet stay inside the row
    for (long k = 0; k < 200000; ++k) {
        const int n = (int)draw(1, 5000), s = (int)draw(1, n);
        const double sh = chance(80) ? (double)draw(0, n) : (double)draw(0, 2 * (int64_t)n) / 2.0;
        double c = chance(70) ? (double)draw(-2 * (int64_t)n, 4 * (int64_t)n) / 2.0 : wild_number(n);
        if (c != c) c = 0.25 + (double)draw(-n, n);
        const AlignWindow w = dsp_align_window(c, sh, s, n);
        const bool ok = w.kind >= 0 && w.kind <= 3 && (w.kind != 1 || (w.first >= 0 && w.first + s <= n)) &&
                        (w.kind != 2 || (w.fill >= 0 && w.fill <= s && w.count >= 0 && w.count <= n && (w.count == 1 || w.fill + w.count == s)));
        if (!ok) {
            std::printf("window of c = %g, shift = %g, size = %d in %d samples: kind %d, first %d, fill %d, count %d\n", c, sh, s, n, w.kind, w.first, w.fill, w.count);
            return 1;
        }
    }
    for (long number = 0; number < programs; ++number) {
        const Prog p = draw_program();
        const char* why = nullptr;
        const std::unique_ptr<ChainPlan> plan = plan_or_refuse(number, p, &why);
        if (!plan) {
            const bool s = std::strstr(why, "(inl_correction, get_wf_centroid, wf_alignment, wf_correction) run on dsp_align_kernel only") != nullptr;
            const bool c = std::strstr(why, "shift ") == why || std::strstr(why, "size ") == why || std::strstr(why, "start_idx ") == why || std::strstr(why, "stop_idx ") == why ||
                           std::strstr(why, "centroid is nan") == why;
            shape += s, checks += c;
            if (s || c || std::strstr(why, "inl_correction") || std::strstr(why, "get_wf_centroid") || std::strstr(why, "wf_alignment") || std::strstr(why, "wf_correction") ||
                std::strstr(why, "INL_CORRECTION") || std::strstr(why, "WF_"))
                ++by_name;
            continue;
        }
        if (!check(number, p, *plan)) return 1;
        if (holds_op(p)) {
            const AlignArgs& A = plan->only.align;
            ++accepted;
            ++kinds[A.correct ? 4 : A.mode - 1];
            aligned_stored += A.correct && plan->bound_io(plan->only.align.out) >= 0;
            per_event += A.mode == DSP_ALIGN_WINDOW && plan->bound_io(plan->only.align.centroid) >= 0;
            ints += integer_rows(plan->only_src.dtype);
        }
    }
    std::printf("{\"programs\": %ld, \"accepted\": %ld, \"inl\": %ld, \"centroid\": %ld, \"align\": %ld, \"correct\": %ld, \"fused\": %ld, \"aligned_stored\": %ld, "
                "\"per_event\": %ld, \"integer_rows\": %ld, \"refused_by_name\": %ld, \"refused_shape\": %ld, \"refused_check\": %ld}\n",
                programs, accepted, kinds[0], kinds[1], kinds[2], kinds[3], kinds[4], aligned_stored, per_event, ints, by_name, shape, checks);
    return 0;
}
