// planner_fuzz.cpp -- test infrastructure: random programs through the device-free planner (dspeed_amd/csrc/dsp_plan.cpp), built for the
// CPU with -fsanitize=address,undefined by tests/test_planner_fuzz.py.
//
//   planner_fuzz <programs> <seed> [digest]
//
// Two kinds of programs: (1) op lists drawn from every opcode with operands that are valid most of the time (so that the validation, the
// constant evaluation and the LDS packing behind it are reached) and garbage some of the time (so that the validation itself is); (2) the
// shapes of the specialised kernels (energy chain, lane-per-waveform rows, matrix-core FIR, pole-zero rows, reductions, current branch, the
// peak finder, the histogram and the threshold kernels)
// with random lengths, offsets, strides and one field mutated.  A program the planner accepts must satisfy its invariants:
//   * LDS: every slot's region inside the wavefront's slot area, regions of slots alive at the same time disjoint, sample 0 behind its
//     zero guard, the register file and the scratch area behind the slots, the whole at most a CU's 160 kB;
//   * a specialised kernel's argument block carries the bindings' offsets and strides (a binding offset is applied, or the shape refused);
//   * the device program's ops stay inside the table, team members are 0 / 1 / 2.
// Exit code 0 and a one-line summary when every program passed; a message and exit code 1 on the first violated invariant (the sanitizers
// end the process themselves).
//
// With `digest` the summary also carries a 64-bit FNV-1a hash over every program's outcome -- the code and message of a refusal; of a plan
// every field the host or a kernel later reads -- so that two builds of the planner can be compared program by program: a refactoring of
// dsp_plan.cpp must print the digest its parent printed, for every seed and under every DSPEED_HIP_* switch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <type_traits>
#include <vector>

#include "../dspeed_amd/csrc/dsp_plan.h"
#include "plan_fuzz_launch.h"

namespace {

std::mt19937_64 rng;
int rnd(int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); }  // inclusive
bool chance(double p) { return (double)(rng() >> 11) * (1.0 / 9007199254740992.0) < p; }
template <typename T>
T pick(std::initializer_list<T> v) { return *(v.begin() + rnd(0, (int)v.size() - 1)); }

struct Prog {
    std::vector<dsp_op> ops;
    std::vector<dsp_io_desc> io;
    std::vector<int32_t> slots;
    int n_sregs = 0;
    int dtype = DSP_F32;
};

int wild() { return pick({-1, 0, 1, 7, 64, 1000, 70000, -2147483647 - 1, 2147483647, rnd(-40, 400)}); }

int add_io(Prog& p, int kind, int dtype, int len, int offset, int64_t stride) {
    dsp_io_desc d{};
    d.kind = kind, d.dtype = dtype, d.len = len, d.offset = offset, d.row_stride = stride;
    p.io.push_back(d);
    return (int)p.io.size() - 1;
}
int scalar_in(Prog& p) { return add_io(p, DSP_IO_SCALAR_IN, pick({DSP_F32, DSP_F32, DSP_F64, DSP_I16, DSP_U16, DSP_I32, DSP_U32}), 1, chance(0.1) ? rnd(0, 3) : 0, pick({1, 1, 1, 0, 2})); }
int scalar_out(Prog& p) { return add_io(p, DSP_IO_SCALAR_OUT, chance(0.1) ? DSP_BOOL : p.dtype, 1, chance(0.1) ? rnd(0, 3) : 0, pick({1, 1, 2})); }
int new_sregs(Prog& p, int n) {
    const int r = p.n_sregs;
    p.n_sregs += n;
    return r;
}
dsp_scalar_arg sarg(Prog& p) {
    dsp_scalar_arg a{};
    const int k = rnd(0, 9);
    if (k < 5 || (k >= 8 && p.n_sregs == 0)) {
        a.kind = DSP_ARG_CONST;
        a.value = pick({0.0, 1.0, -1.0, 0.5, 3.0, 16.0, 100.25, 1716.28, 1e30, -1e30, (double)NAN, (double)INFINITY, (double)rnd(-50, 5000)});
    } else if (k < 8) {
        a.kind = DSP_ARG_INPUT;
        a.index = scalar_in(p);
    } else {
        a.kind = DSP_ARG_REG;
        a.index = rnd(0, p.n_sregs - 1);
    }
    if (chance(0.01)) a.kind = rnd(-1, 4);
    if (chance(0.01)) a.index = wild();
    return a;
}
dsp_scalar_arg f32_col(Prog& p) {
    dsp_scalar_arg a{};
    a.kind = DSP_ARG_INPUT;
    a.index = add_io(p, DSP_IO_SCALAR_IN, DSP_F32, 1, 0, pick({1, 1, 1, 0, 2}));
    return a;
}
dsp_scalar_arg cst(double v);
// operand of a specialised shape: what the kernels take (a finite constant, a float32 column) four times out of five
dsp_scalar_arg shape_arg(Prog& p) { return chance(0.4) ? f32_col(p) : chance(0.67) ? cst(pick({0.0, 1.0, 12.5, 100.0, 1716.28, 4000.0})) : sarg(p); }
int f32_out(Prog& p) { return chance(0.9) ? add_io(p, DSP_IO_SCALAR_OUT, DSP_F32, 1, 0, 1) : scalar_out(p); }
dsp_scalar_arg cst(double v) {
    dsp_scalar_arg a{};
    a.kind = DSP_ARG_CONST;
    a.value = v;
    return a;
}
int in_dtype(const Prog& p) { return p.dtype == DSP_F64 ? pick({DSP_F64, DSP_I32, DSP_U32, DSP_F32, DSP_I16, DSP_U16}) : pick({DSP_F32, DSP_F32, DSP_I16, DSP_U16}); }
int new_slot(Prog& p, int len) {
    p.slots.push_back(len);
    return (int)p.slots.size() - 1;
}
int some_len() { return pick({1, 2, 3, 4, 8, 16, 63, 64, 65, 100, 256, 301, 1000, 1024, 2048, 4096, 4784, 6092, 8192, rnd(1, 9000)}); }
int any_slot(Prog& p) { return p.slots.empty() ? 0 : rnd(0, (int)p.slots.size() - 1); }
dsp_op op0(int opcode) {
    dsp_op o{};
    o.opcode = opcode;
    return o;
}
int load_slot(Prog& p, int len) {  // LOAD of a fresh slot from a fresh input binding
    const int s = new_slot(p, len);
    const int off = chance(0.3) ? rnd(0, 40) : 0;
    const int tail = chance(0.3) ? rnd(0, 40) : 0;
    dsp_op o = op0(DSP_OP_LOAD);
    o.dst = s;
    o.io = add_io(p, DSP_IO_WF_IN, in_dtype(p), len, off, (int64_t)off + len + tail);
    if (chance(0.2)) o.ip[0] = rnd(0, off), o.ip[1] = rnd(0, tail);
    if (chance(0.2)) o.ip[2] = 1;
    p.ops.push_back(o);
    return s;
}

// one random op on the program so far; mostly well-formed
void random_op(Prog& p) {
    if (p.slots.empty() || chance(0.15)) {
        if (p.slots.size() < DSP_MAX_SLOTS) load_slot(p, some_len());
        return;
    }
    const int src = any_slot(p), n = p.slots[src];
    dsp_op o{};
    switch (rnd(0, 27)) {
        case 0: {
            o = op0(DSP_OP_STORE);
            o.src = src;
            o.io = add_io(p, DSP_IO_WF_OUT, chance(0.1) ? DSP_BOOL : p.dtype, n, 0, n + (chance(0.2) ? rnd(0, 9) : 0));
            break;
        }
        case 1: o = op0(DSP_OP_STORE_SCALAR), o.io = scalar_out(p), o.ip[0] = p.n_sregs ? rnd(0, p.n_sregs - 1) : 0; break;
        case 2: o = op0(pick({DSP_OP_BL_SUBTRACT, DSP_OP_MIN_MAX_NORM})), o.src = src, o.dst = chance(0.6) ? src : new_slot(p, n), o.sp[0] = sarg(p), o.sp[1] = sarg(p), o.ip[0] = chance(0.2); break;
        case 3: o = op0(DSP_OP_POLE_ZERO), o.src = src, o.dst = chance(0.6) ? src : new_slot(p, n), o.sp[0] = sarg(p); break;
        case 4: o = op0(DSP_OP_DOUBLE_POLE_ZERO), o.src = src, o.dst = chance(0.6) ? src : new_slot(p, n), o.sp[0] = sarg(p), o.sp[1] = sarg(p), o.sp[2] = sarg(p); break;
        case 5: {
            o = op0(pick({DSP_OP_TRAP_FILTER, DSP_OP_TRAP_NORM, DSP_OP_ASYM_TRAP}));
            o.src = src, o.dst = new_slot(p, n);
            o.ip[0] = rnd(-1, n / 3 + 2), o.ip[1] = rnd(-1, n / 3 + 2), o.ip[2] = rnd(-1, n / 3 + 2);
            break;
        }
        case 6: {
            o = op0(DSP_OP_TRAP_PICKOFF);
            o.src = src, o.dst = new_sregs(p, 1), o.io = pick({'l', 'n', 'f', 'c', 'h', 'i', 's', 'x'});
            o.ip[0] = rnd(0, n / 3 + 1), o.ip[1] = rnd(0, n / 3 + 1), o.ip[2] = rnd(0, n / 3 + 1), o.ip[3] = pick({DSP_OP_TRAP_FILTER, DSP_OP_TRAP_NORM, DSP_OP_ASYM_TRAP, 0});
            o.sp[0] = sarg(p);
            break;
        }
        case 7: {
            o = op0(DSP_OP_TRAP_REDUCE);
            o.src = src, o.dst = chance(0.7) ? new_sregs(p, 4) : -1, o.io = chance(0.6) ? new_sregs(p, 1) : -1;
            int code = pick({DSP_OP_TRAP_FILTER, DSP_OP_TRAP_NORM, DSP_OP_ASYM_TRAP});
            if (chance(0.3)) code |= (pick({'l', 'n', 'i', 'h', 's'}) << 8) | ((new_sregs(p, 1) + 1) << 16);
            if (chance(0.3)) code |= 1 << 30;
            o.ip[0] = rnd(0, n / 3 + 1), o.ip[1] = rnd(0, n / 3 + 1), o.ip[2] = rnd(0, n / 3 + 1), o.ip[3] = code;
            for (int k = 0; k < 4; ++k) o.sp[k] = sarg(p);
            break;
        }
        case 8: {
            o = op0(DSP_OP_PICKOFF);
            o.src = src, o.dst = new_sregs(p, 1), o.ip[0] = pick({'l', 'n', 'f', 'c', 'h', 'i', 's', 'q'}), o.ip[1] = pick({0, 0, 1, 2, 3});
            o.sp[0] = o.ip[1] == 1 ? cst(rnd(-1, n)) : sarg(p), o.sp[1] = chance(0.8) ? cst(NAN) : sarg(p);
            break;
        }
        case 9: o = op0(pick({DSP_OP_TIME_POINT_THRESH, DSP_OP_INTERP_TIME_POINT_THRESH})), o.src = src, o.dst = new_sregs(p, 1), o.ip[0] = pick({'i', 'b', 'c', 'a', 'f', 'r', 'n', 'l', 'z'}), o.sp[0] = sarg(p), o.sp[1] = sarg(p), o.sp[2] = sarg(p); break;
        case 10: o = op0(pick({DSP_OP_MEAN_BELOW, DSP_OP_AMAX})), o.src = src, o.dst = new_sregs(p, 1), o.sp[0] = sarg(p); break;
        case 11: o = op0(pick({DSP_OP_MIN_MAX, DSP_OP_LINEAR_SLOPE_FIT})), o.src = src, o.dst = new_sregs(p, 4), o.ip[0] = chance(0.5) ? rnd(0, n) : 0, o.ip[1] = chance(0.5) ? rnd(0, n) : 0; break;
        case 12: o = op0(DSP_OP_WINDOWER), o.src = src, o.dst = new_slot(p, chance(0.9) ? rnd(1, n > 1 ? n - 1 : 1) : n), o.sp[0] = sarg(p); break;
        case 13: {
            const int L = rnd(0, n > 1 ? n - 1 : 0);
            o = op0(DSP_OP_AVG_CURRENT), o.src = src, o.dst = new_slot(p, chance(0.9) ? (n - L > 0 ? n - L : 1) : some_len()), o.sp[0] = chance(0.9) ? cst(L + (chance(0.3) ? 0.5 : 0.0)) : sarg(p);
            break;
        }
        case 14: {
            const int up = pick({1, 2, 4, 8, 16, 3, 0, -1});
            o = op0(DSP_OP_UPSAMPLER), o.src = src, o.dst = new_slot(p, chance(0.9) && up > 0 && (int64_t)n * up < 20000 ? n * up : some_len()), o.sp[0] = chance(0.9) ? cst(up) : sarg(p);
            break;
        }
        case 15: {
            o = op0(DSP_OP_MOVING_WINDOW_MULTI);
            const int win = pick({1, 3, 16, 48, 112, 0, -1, rnd(1, n)}), num = pick({0, 1, 2, 3, 4, -1});
            o.src = src, o.sp[0] = chance(0.9) ? cst(win + (chance(0.05) ? 0.5 : 0.0)) : sarg(p), o.ip[0] = pick({0, 1, 2}), o.ip[1] = num;
            if (chance(0.3)) {
                o.dst = src, o.ip[3] = 1, o.ip[2] = new_slot(p, chance(0.9) && win > 0 ? 64 * win : some_len());
            } else {
                o.dst = new_slot(p, n), o.ip[2] = chance(0.8) ? new_slot(p, n) : any_slot(p);
            }
            break;
        }
        case 16: o = op0(DSP_OP_TRAP_WINDOW_PICKOFF), o.src = src, o.dst = new_sregs(p, 1), o.ip[0] = rnd(-1, n / 2 + 1), o.ip[1] = rnd(-1, n / 2 + 1), o.sp[0] = sarg(p); break;
        case 17: {
            const int level = rnd(0, 9);
            int len = n;
            for (int l = 0; l < level; ++l) len = (len + 1) / 2;
            o = op0(DSP_OP_DWT_HAAR), o.src = src, o.dst = new_slot(p, chance(0.9) ? (len > 0 ? len : 1) : some_len()), o.ip[0] = level, o.ip[1] = pick({'a', 'd', 'a', 'x'});
            o.ip[2] = chance(0.5) ? src : new_slot(p, chance(0.9) ? n : some_len());
            break;
        }
        case 18: {
            const int step = pick({1, 1, 2, 3, -1, -2, 0}), first = rnd(0, n - 1);
            const int cnt = step >= 0 ? (n - first + (step ? step : 1) - 1) / (step ? step : 1) : first / -step + 1;
            o = op0(DSP_OP_COPY), o.src = src, o.dst = new_slot(p, chance(0.9) ? (cnt > 0 ? rnd(1, cnt) : 1) : some_len()), o.ip[0] = first, o.ip[1] = step;
            break;
        }
        case 19: {
            o = op0(DSP_OP_ELEMENTWISE);
            int fn = rnd(0, DSP_FN_LAST + 1);
            if (fn >= DSP_FN_IADD && fn <= DSP_FN_ICAST) fn |= DSP_FN_INT(pick({8, 16, 32, 64, 0}), chance(0.5));
            o.ip[0] = fn, o.src = chance(0.8) ? src : -1, o.ip[1] = chance(0.4) ? src : -1, o.ip[2] = chance(0.2) ? any_slot(p) : -1;
            o.dst = chance(0.5) ? src : new_slot(p, n);
            for (int k = 0; k < 3; ++k) o.sp[k] = sarg(p);
            break;
        }
        case 20: {
            o = op0(DSP_OP_SCALAR_FUNC);
            int fn = rnd(0, DSP_FN_LAST + 1);
            if (fn >= DSP_FN_IADD && fn <= DSP_FN_ICAST) fn |= DSP_FN_INT(pick({8, 16, 32, 64}), chance(0.5));
            o.ip[0] = fn, o.dst = new_sregs(p, 1);
            for (int k = 0; k < 3; ++k) o.sp[k] = sarg(p);
            break;
        }
        case 21:
        case 22: {
            const int mode = pick({'v', 's', 'f', 'v', 'x'}), m = rnd(1, n + 2);
            const int outlen = mode == 'v' ? n - m + 1 : mode == 's' ? n : n + m - 1;
            o = op0(pick({DSP_OP_CONVOLVE, DSP_OP_CONVOLVE_AMAX}));
            const int padded = ((m + 15) / 16) * 16;
            o.src = src, o.io = add_io(p, DSP_IO_TAPS, p.dtype, chance(0.7) ? padded : m, 0, 0), o.ip[0] = mode, o.ip[1] = rnd(0, 3), o.ip[3] = chance(0.7) ? m : 0;
            if (o.opcode == DSP_OP_CONVOLVE) o.dst = new_slot(p, chance(0.9) && outlen > 0 ? outlen : some_len());
            else o.dst = new_sregs(p, 1), o.ip[2] = chance(0.9) ? outlen : wild();
            break;
        }
        case 23: o = op0(DSP_OP_SCALAR_AFFINE), o.dst = new_sregs(p, 1), o.sp[0] = sarg(p), o.sp[1] = sarg(p), o.sp[2] = sarg(p); break;
        case 24: o = op0(DSP_OP_SCALAR_DIV), o.dst = new_sregs(p, 1), o.sp[0] = sarg(p), o.sp[1] = sarg(p); break;
        case 25: o = op0(DSP_OP_SCALAR_CONVERT), o.dst = new_sregs(p, 1), o.ip[0] = rnd(0, 4), o.sp[0] = sarg(p), o.sp[1] = sarg(p), o.sp[2] = sarg(p), o.sp[3] = cst(pick({1.0, 16.0, 0.0625})); break;
        default: o = op0(rnd(-2, 40)), o.dst = wild(), o.src = wild(), o.io = wild(); break;
    }
    // now and then: garbage in one field
    if (chance(0.03)) o.dst = wild();
    if (chance(0.03)) o.src = wild();
    if (chance(0.03)) o.io = wild();
    if (chance(0.03)) o.ip[rnd(0, 3)] = wild();
    if (p.slots.size() > DSP_MAX_SLOTS) p.slots.resize(DSP_MAX_SLOTS);
    p.ops.push_back(o);
}

Prog random_program() {
    Prog p;
    p.dtype = chance(0.25) ? DSP_F64 : DSP_F32;
    const int n = rnd(1, chance(0.1) ? 60 : 14);
    for (int i = 0; i < n && (int)p.ops.size() < DSP_MAX_OPS && (int)p.io.size() < DSP_MAX_IO - 8 && p.n_sregs < DSP_MAX_SREGS - 8; ++i) random_op(p);
    if (p.ops.empty()) random_op(p);
    return p;
}

// ---- the specialised kernels' shapes, with random geometry
Prog energy_shape() {
    Prog p;
    const int len = pick({1024, 2048, 4096, 8192, 4096, 1000, 512});
    const int off = pick({0, 0, 0, 4, 8, 3}), stride = off + len + pick({0, 0, 0, 4, 16, 1});
    const int s = new_slot(p, len), r = new_sregs(p, 1);
    dsp_op ld = op0(DSP_OP_LOAD);
    ld.dst = s, ld.io = add_io(p, DSP_IO_WF_IN, pick({DSP_F32, DSP_I16, DSP_U16}), len, off, stride);
    p.ops.push_back(ld);
    if (chance(0.8)) {
        dsp_op b = op0(DSP_OP_BL_SUBTRACT);
        b.dst = b.src = s, b.sp[0] = shape_arg(p);
        p.ops.push_back(b);
    }
    dsp_op pz = op0(DSP_OP_POLE_ZERO);
    pz.dst = pz.src = s, pz.sp[0] = chance(0.7) ? cst(1716.28) : shape_arg(p);
    p.ops.push_back(pz);
    dsp_op tp = op0(DSP_OP_TRAP_PICKOFF);
    tp.dst = r, tp.src = s, tp.io = pick({'l', 'n', 'h', 'i', 'f', 'c'}), tp.ip[0] = rnd(0, len / 3), tp.ip[1] = rnd(0, len / 3), tp.ip[3] = pick({DSP_OP_TRAP_FILTER, DSP_OP_TRAP_NORM}), tp.sp[0] = shape_arg(p);
    p.ops.push_back(tp);
    dsp_op st = op0(DSP_OP_STORE_SCALAR);
    st.io = f32_out(p), st.ip[0] = r;
    p.ops.push_back(st);
    return p;
}

Prog rows_shape() {
    Prog p;
    const int len = pick({8192, 4096, 1024, 64, 1000, 8200});
    const int off = pick({0, 0, 8, 16, 2}), stride = off + len + pick({0, 8, 1});
    const int s = new_slot(p, len);
    dsp_op ld = op0(DSP_OP_LOAD);
    ld.dst = s, ld.io = add_io(p, DSP_IO_WF_IN, pick({DSP_F32, DSP_I16, DSP_U16}), len, off, stride), ld.ip[2] = chance(0.3);
    p.ops.push_back(ld);
    if (chance(0.3)) {
        dsp_op b = op0(DSP_OP_BL_SUBTRACT);
        b.dst = b.src = s, b.sp[0] = shape_arg(p);
        p.ops.push_back(b);
    }
    int wf = s;
    if (chance(0.7)) {
        dsp_op z = op0(pick({DSP_OP_POLE_ZERO, DSP_OP_DOUBLE_POLE_ZERO}));
        z.dst = z.src = s, z.sp[0] = cst(1716.28), z.sp[1] = cst(62.5), z.sp[2] = cst(0.02);
        p.ops.push_back(z);
    }
    if (chance(0.4)) {
        const int level = rnd(2, 9), d = new_slot(p, (len >> level) > 0 ? len >> level : 1);
        dsp_op w = op0(DSP_OP_DWT_HAAR);
        w.src = wf, w.dst = d, w.ip[0] = level, w.ip[1] = pick({'a', 'd'}), w.ip[2] = wf;
        p.ops.push_back(w);
        dsp_op st = op0(DSP_OP_STORE);
        st.src = d, st.io = add_io(p, DSP_IO_WF_OUT, DSP_F32, p.slots[d], pick({0, 4, 1}), p.slots[d] + pick({0, 4, 1}) + 4);
        p.ops.push_back(st);
    }
    dsp_op tr = op0(DSP_OP_TRAP_REDUCE);
    tr.src = wf, tr.dst = chance(0.7) ? new_sregs(p, 4) : -1, tr.io = chance(0.7) ? new_sregs(p, 1) : -1;
    tr.ip[0] = pick({8, 16, 4, 100}), tr.ip[1] = pick({4, 8, 0}), tr.ip[2] = pick({125, 8, 400}), tr.ip[3] = pick({DSP_OP_TRAP_FILTER, DSP_OP_TRAP_NORM, DSP_OP_ASYM_TRAP});
    tr.sp[0] = shape_arg(p), tr.sp[1] = (tr.dst >= 0 && chance(0.5)) ? dsp_scalar_arg{DSP_ARG_REG, tr.dst + rnd(0, 1), 0.0} : shape_arg(p), tr.sp[2] = cst(pick({0.0, 1.0, 0.0, 1.0, 0.5, (double)NAN}));
    p.ops.push_back(tr);
    for (int k = 0; k < 4 && tr.dst >= 0; ++k)
        if (chance(0.7)) {
            dsp_op st = op0(DSP_OP_STORE_SCALAR);
            st.io = f32_out(p), st.ip[0] = tr.dst + k;
            p.ops.push_back(st);
        }
    if (tr.io >= 0) {
        dsp_op st = op0(DSP_OP_STORE_SCALAR);
        st.io = f32_out(p), st.ip[0] = tr.io;
        p.ops.push_back(st);
    }
    return p;
}

Prog fir_shape() {
    Prog p;
    const int full = pick({8192, 4096, 1000}), off = pick({0, 0, 8, 100, 3}), n = pick({6092, 4000, 512, full - off});
    const int len = n > 0 && off + n <= full ? n : full - off;
    const int s = new_slot(p, len);
    dsp_op ld = op0(DSP_OP_LOAD);
    ld.dst = s, ld.io = add_io(p, DSP_IO_WF_IN, pick({DSP_F32, DSP_I16, DSP_U16}), len, off, full);
    if (chance(0.5)) ld.ip[0] = off, ld.ip[1] = full - off - len;
    p.ops.push_back(ld);
    if (chance(0.6)) {
        dsp_op b = op0(DSP_OP_BL_SUBTRACT);
        b.dst = b.src = s, b.sp[0] = shape_arg(p);
        p.ops.push_back(b);
    }
    const bool store = chance(0.4);
    const int nk = store ? 1 : rnd(1, 5);
    for (int k = 0; k < nk; ++k) {
        const int m = pick({64, 133, 5792, 300, 63, len, len + 1}), mode = store ? pick({'v', 's', 'f'}) : 'v';
        const int outlen = mode == 'v' ? len - m + 1 : mode == 's' ? len : len + m - 1;
        const int padded = ((m + 15) / 16) * 16;
        dsp_op c = op0(store ? DSP_OP_CONVOLVE : DSP_OP_CONVOLVE_AMAX);
        c.src = s, c.io = add_io(p, DSP_IO_TAPS, DSP_F32, padded, 0, 0), c.ip[0] = mode, c.ip[1] = chance(0.1) ? rnd(1, 3) : 0, c.ip[3] = m;
        if (store) {
            c.dst = new_slot(p, outlen > 0 ? outlen : 1);
            p.ops.push_back(c);
            dsp_op st = op0(DSP_OP_STORE);
            st.src = c.dst, st.io = add_io(p, DSP_IO_WF_OUT, DSP_F32, p.slots[c.dst], pick({0, 0, 4}), p.slots[c.dst] + 8);
            p.ops.push_back(st);
        } else {
            c.dst = new_sregs(p, 1), c.ip[2] = outlen;
            p.ops.push_back(c);
            dsp_op st = op0(DSP_OP_STORE_SCALAR);
            st.io = f32_out(p), st.ip[0] = c.dst;
            p.ops.push_back(st);
        }
    }
    return p;
}

// LOAD, CONVOLVE with the piecewise-constant hint, [STORE], [reductions of the filtered waveform] (dsp_fir_runs.hip)
Prog fir_runs_shape() {
    Prog p;
    const int len = pick({8192, 4096, 1000, 512, 8}), off = pick({0, 0, 8, 4, 1}), stride = off + len + pick({0, 8, 3});
    const int s = new_slot(p, len);
    dsp_op ld = op0(DSP_OP_LOAD);
    ld.dst = s, ld.io = add_io(p, DSP_IO_WF_IN, pick({DSP_F32, DSP_F32, DSP_F32, DSP_I16}), len, off, stride);
    if (chance(0.1)) ld.ip[0] = off;
    p.ops.push_back(ld);
    const int m = pick({133, 16, 1, 512, 513, 64, len}), mode = pick({'v', 's', 'f', 'x'});
    const int outlen = mode == 'v' ? len - m + 1 : mode == 's' ? len : len + m - 1;
    dsp_op c = op0(DSP_OP_CONVOLVE);
    c.src = s, c.dst = new_slot(p, outlen > 0 ? outlen : 1), c.io = add_io(p, DSP_IO_TAPS, DSP_F32, ((m + 15) / 16) * 16, 0, 0);
    c.ip[0] = mode, c.ip[1] = chance(0.1) ? rnd(1, 3) : 0, c.ip[2] = chance(0.9) ? 1 : rnd(0, 2), c.ip[3] = m;
    p.ops.push_back(c);
    const bool keep = chance(0.5), store_first = chance(0.5);
    dsp_op st = op0(DSP_OP_STORE);
    st.src = c.dst, st.io = add_io(p, DSP_IO_WF_OUT, DSP_F32, p.slots[c.dst], pick({0, 0, 4}), p.slots[c.dst] + 8);
    if (keep && store_first) p.ops.push_back(st);
    int mm = -1;
    std::vector<int> regs;
    for (int k = rnd(keep ? 0 : 1, 5); k > 0; --k) {
        dsp_op o{};
        switch (rnd(0, 3)) {
            case 0: o = op0(DSP_OP_MIN_MAX), o.src = c.dst, o.dst = mm = new_sregs(p, 4); for (int q = 0; q < 4; ++q) regs.push_back(mm + q); break;
            case 1: o = op0(DSP_OP_AMAX), o.src = c.dst, o.dst = new_sregs(p, 1), regs.push_back(o.dst); break;
            case 2: o = op0(DSP_OP_PICKOFF), o.src = c.dst, o.dst = new_sregs(p, 1), o.ip[0] = pick({'i', 'l', 'n'}), o.ip[1] = pick({0, 1}), o.sp[0] = cst(pick({0.0, 50.0, 50.5, (double)outlen, -1.0})), regs.push_back(o.dst); break;
            default:
                o = op0(DSP_OP_TIME_POINT_THRESH), o.src = c.dst, o.dst = new_sregs(p, 1), o.sp[0] = shape_arg(p);
                o.sp[1] = (mm >= 0 && chance(0.5)) ? dsp_scalar_arg{DSP_ARG_REG, mm + rnd(0, 1), 0.0} : cst(pick({0.0, 100.0, 100.5, -1.0}));
                o.sp[2] = cst(pick({0.0, 1.0, 0.5}));
                regs.push_back(o.dst);
        }
        p.ops.push_back(o);
    }
    for (int r : regs)
        if (chance(0.9)) {
            dsp_op sc = op0(DSP_OP_STORE_SCALAR);
            sc.io = f32_out(p), sc.ip[0] = r;
            p.ops.push_back(sc);
        }
    if (keep && !store_first) p.ops.push_back(st);
    return p;
}

Prog pz_shape() {
    Prog p;
    const int len = pick({8192, 4096, 1000, 8}), off = pick({0, 0, 8, 4, 1}), stride = off + len + pick({0, 8, 3});
    const int s = new_slot(p, len);
    dsp_op ld = op0(DSP_OP_LOAD);
    ld.dst = s, ld.io = add_io(p, DSP_IO_WF_IN, pick({DSP_F32, DSP_I16, DSP_U16}), len, off, stride);
    p.ops.push_back(ld);
    int mm = -1;
    if (chance(0.4)) {  // min_max of the rows as they are read
        dsp_op m = op0(DSP_OP_MIN_MAX);
        m.src = s, m.dst = mm = new_sregs(p, 4);
        p.ops.push_back(m);
    }
    if (chance(0.6)) {
        dsp_op b = op0(DSP_OP_BL_SUBTRACT);
        b.dst = b.src = s, b.sp[0] = shape_arg(p);
        p.ops.push_back(b);
    }
    dsp_op pz = op0(DSP_OP_POLE_ZERO);
    pz.dst = pz.src = s, pz.sp[0] = chance(0.7) ? cst(pick({1716.28, 1716.28, 0.0, (double)NAN})) : shape_arg(p);
    p.ops.push_back(pz);
    const bool stores_first = chance(0.5);
    auto stores = [&]() {
        for (int k = 0; mm >= 0 && k < 4; ++k)
            if (chance(0.85)) {
                dsp_op sc = op0(DSP_OP_STORE_SCALAR);
                sc.io = f32_out(p), sc.ip[0] = mm + k;
                p.ops.push_back(sc);
            }
    };
    if (stores_first) stores();
    dsp_op st = op0(DSP_OP_STORE);
    const int ooff = pick({0, 0, 4, 1});
    st.src = s, st.io = add_io(p, DSP_IO_WF_OUT, DSP_F32, len, ooff, ooff + len + pick({0, 4}));
    p.ops.push_back(st);
    if (!stores_first) stores();
    return p;
}

Prog reduce_shape() {
    Prog p;
    const int len = pick({8192, 4096, 301, 1000}), off = pick({0, 0, 8, 3}), stride = off + len + pick({0, 8, 1});
    const int s = new_slot(p, len);
    dsp_op ld = op0(DSP_OP_LOAD);
    ld.dst = s, ld.io = add_io(p, DSP_IO_WF_IN, pick({DSP_F32, DSP_I16, DSP_U16}), len, off, stride);
    p.ops.push_back(ld);
    int mm = -1, last_walk = -1;
    std::vector<int> regs;
    ld.ip[2] = chance(0.5);  // (the promise about the rows' NaNs: walks alone then need no pass over the row)
    p.ops[0] = ld;
    for (int k = rnd(1, 8); k > 0; --k) {
        dsp_op o{};
        switch (rnd(0, 3)) {
            case 0: o = op0(DSP_OP_MIN_MAX), o.src = s, o.dst = mm = new_sregs(p, 4); for (int q = 0; q < 4; ++q) regs.push_back(mm + q); break;
            case 1: o = op0(DSP_OP_AMAX), o.src = s, o.dst = new_sregs(p, 1), regs.push_back(o.dst); break;
            case 2: o = op0(DSP_OP_PICKOFF), o.src = s, o.dst = new_sregs(p, 1), o.ip[0] = pick({'i', 'l', 'n'}), o.ip[1] = pick({0, 1}), o.sp[0] = cst(pick({0.0, 50.0, 50.5, (double)len, -1.0})), regs.push_back(o.dst); break;
            default: {
                // a threshold: a constant, a column, a fraction of a column (SCALAR_AFFINE in front); a start: a constant, an extreme, a column,
                // where an earlier walk ended
                dsp_scalar_arg thr = shape_arg(p);
                if (chance(0.3)) {
                    dsp_op a = op0(DSP_OP_SCALAR_AFFINE);
                    a.dst = new_sregs(p, 1), a.sp[0] = shape_arg(p), a.sp[1] = cst(pick({0.9, 0.5, 1.0})), a.sp[2] = cst(pick({0.0, 0.0, -0.0, 1.0}));
                    p.ops.push_back(a);
                    thr = dsp_scalar_arg{DSP_ARG_REG, a.dst, 0.0};
                }
                o = op0(DSP_OP_TIME_POINT_THRESH), o.src = s, o.dst = new_sregs(p, 1), o.sp[0] = thr;
                if (mm >= 0 && chance(0.3)) o.sp[1] = dsp_scalar_arg{DSP_ARG_REG, mm + rnd(0, 1), 0.0};
                else if (last_walk >= 0 && chance(0.4)) o.sp[1] = dsp_scalar_arg{DSP_ARG_REG, last_walk, 0.0};
                else if (chance(0.3)) o.sp[1] = shape_arg(p);
                else o.sp[1] = cst(pick({0.0, 100.0, 100.5, -1.0}));
                o.sp[2] = cst(pick({0.0, 1.0, 0.5}));
                regs.push_back(o.dst);
                last_walk = o.dst;
            }
        }
        p.ops.push_back(o);
    }
    for (int r : regs)
        if (chance(0.9)) {
            dsp_op st = op0(DSP_OP_STORE_SCALAR);
            st.io = f32_out(p), st.ip[0] = r;
            p.ops.push_back(st);
        }
    return p;
}

Prog current_shape() {
    Prog p;
    const int len = pick({8192, 4096}), off = pick({0, 0, 4, 1}), stride = off + len + pick({0, 4});
    const int win = pick({301, 301, 101, 300}), lag = pick({1, 1, 2, 0}), up = pick({16, 16, 8, 1, 3}), ma = pick({48, 48, 16, 112, 40, 128});
    const int reach = (win - lag) * up - up / 2;  // upsampled samples an input sample lands on
    const int s = new_slot(p, len), w = new_slot(p, win), c = new_slot(p, win - lag), u = new_slot(p, pick({reach / 16 * 16, reach / 16 * 16, (win - lag) * up, 4784}));
    dsp_op ld = op0(DSP_OP_LOAD);
    ld.dst = s, ld.io = add_io(p, DSP_IO_WF_IN, pick({DSP_F32, DSP_F32, DSP_F32, DSP_I16}), len, off, stride), ld.ip[2] = chance(0.5);
    p.ops.push_back(ld);
    dsp_op a = op0(DSP_OP_WINDOWER);
    a.src = s, a.dst = w, a.sp[0] = shape_arg(p);
    p.ops.push_back(a);
    dsp_op b = op0(DSP_OP_AVG_CURRENT);
    b.src = w, b.dst = c, b.sp[0] = cst(lag);
    p.ops.push_back(b);
    dsp_op d = op0(DSP_OP_UPSAMPLER);
    d.src = c, d.dst = u, d.sp[0] = cst(up);
    p.ops.push_back(d);
    dsp_op m = op0(DSP_OP_MOVING_WINDOW_MULTI);
    const bool inplace = chance(0.6);
    m.src = u, m.dst = inplace ? u : new_slot(p, p.slots[u]), m.sp[0] = cst(ma), m.ip[0] = pick({0, 0, 0, 1}), m.ip[1] = pick({3, 3, 3, 2, 1});
    m.ip[2] = inplace ? new_slot(p, 64 * ma) : u, m.ip[3] = inplace;
    p.ops.push_back(m);
    dsp_op mmx = op0(DSP_OP_MIN_MAX);
    mmx.src = m.dst, mmx.dst = new_sregs(p, 4);
    p.ops.push_back(mmx);
    for (int k = 0; k < 4; ++k)
        if (chance(0.8)) {
            dsp_op st = op0(DSP_OP_STORE_SCALAR);
            st.io = f32_out(p), st.ip[0] = mmx.dst + k;
            p.ops.push_back(st);
        }
    return p;
}

// arithmetic between per-event values and stores only: the row-per-lane kernel's programs (the tail of a recipe)
// an integer program (compute type DSP_I64, dspeed_hip.h): SCALAR_FUNC and STORE_SCALAR ops only, integer / bool input columns, outputs of any type
Prog integer_shape() {
    Prog p;
    p.dtype = DSP_I64;
    auto in_col = [&]() {
        dsp_scalar_arg a{};
        a.kind = DSP_ARG_INPUT;
        a.index = add_io(p, DSP_IO_SCALAR_IN, chance(0.02) ? DSP_F32 : pick({DSP_I64, DSP_U64, DSP_I32, DSP_U32, DSP_I16, DSP_U16, DSP_BOOL, DSP_I64}), 1, 0, pick({1, 1, 0, 2}));
        return a;
    };
    auto opnd = [&]() {
        if (p.n_sregs && chance(0.4)) return dsp_scalar_arg{DSP_ARG_REG, rnd(0, p.n_sregs - 1), 0.0};
        if (chance(0.5)) return in_col();
        return cst((double)pick({0, 1, -1, 7, 65535, 1 << 30, rnd(-1000, 1000)}));
    };
    for (int k = rnd(1, 30); k > 0 && p.n_sregs < DSP_MAX_SREGS - 4 && (int)p.io.size() < DSP_MAX_IO - 6; --k) {
        dsp_op o{};
        if (p.n_sregs && chance(0.3)) {
            o = op0(DSP_OP_STORE_SCALAR);
            o.io = add_io(p, DSP_IO_SCALAR_OUT, pick({DSP_I64, DSP_U64, DSP_I32, DSP_U32, DSP_I16, DSP_U16, DSP_BOOL, DSP_F32, DSP_F64}), 1, 0, 1);
            o.ip[0] = rnd(0, p.n_sregs - 1), o.ip[1] = chance(0.2);
        } else {
            int fn = pick({DSP_FN_IADD, DSP_FN_ISUB, DSP_FN_IMUL, DSP_FN_IFLOORDIV, DSP_FN_ICAST, DSP_FN_LT, DSP_FN_GE, DSP_FN_EQ, DSP_FN_WHERE, DSP_FN_LOR, DSP_FN_LAND, DSP_FN_COPY});
            if (chance(0.02)) fn = pick({DSP_FN_ADD, DSP_FN_RINT, DSP_FN_DIV});  // (float functions: refused in an integer program)
            if (fn >= DSP_FN_IADD && fn <= DSP_FN_ICAST) fn |= DSP_FN_INT(chance(0.02) ? 24 : pick({8, 16, 32, 64, 64}), chance(0.5));
            else if (chance(0.3)) fn |= DSP_FN_INT(64, chance(0.5));
            o = op0(chance(0.97) ? DSP_OP_SCALAR_FUNC : DSP_OP_SCALAR_AFFINE), o.ip[0] = fn;
            for (int q = 0; q < 3; ++q) o.sp[q] = opnd();
            o.dst = new_sregs(p, 1);
        }
        p.ops.push_back(o);
    }
    if (p.ops.empty()) p.ops.push_back(op0(DSP_OP_SCALAR_FUNC)), p.n_sregs = 1;
    return p;
}

Prog scalar_shape() {
    if (chance(0.3)) return integer_shape();
    Prog p;
    p.dtype = chance(0.3) ? DSP_F64 : DSP_F32;
    for (int k = rnd(1, 40); k > 0 && p.n_sregs < DSP_MAX_SREGS - 4 && (int)p.io.size() < DSP_MAX_IO - 6; --k) {
        dsp_op o{};
        switch (rnd(0, 4)) {
            case 0: o = op0(DSP_OP_SCALAR_AFFINE), o.sp[0] = sarg(p), o.sp[1] = sarg(p), o.sp[2] = sarg(p), o.dst = new_sregs(p, 1); break;
            case 1: o = op0(DSP_OP_SCALAR_DIV), o.sp[0] = sarg(p), o.sp[1] = sarg(p), o.dst = new_sregs(p, 1); break;
            case 2: o = op0(DSP_OP_SCALAR_CONVERT), o.ip[0] = rnd(0, 4), o.sp[0] = sarg(p), o.sp[1] = sarg(p), o.sp[2] = sarg(p), o.sp[3] = cst(pick({1.0, 16.0, 0.0625})), o.dst = new_sregs(p, 1); break;
            case 3: {
                int fn = rnd(0, DSP_FN_LAST);
                if (fn >= DSP_FN_IADD && fn <= DSP_FN_ICAST) fn |= DSP_FN_INT(pick({8, 16, 32}), chance(0.5));
                o = op0(DSP_OP_SCALAR_FUNC), o.ip[0] = fn;
                for (int q = 0; q < 3; ++q) o.sp[q] = sarg(p);
                o.dst = new_sregs(p, 1);
                break;
            }
            default:
                if (!p.n_sregs) continue;
                o = op0(DSP_OP_STORE_SCALAR), o.io = scalar_out(p), o.ip[0] = rnd(0, p.n_sregs - 1);
        }
        p.ops.push_back(o);
    }
    if (p.ops.empty()) p.ops.push_back(op0(DSP_OP_SCALAR_AFFINE)), p.n_sregs = 1;
    return p;
}

// ---- the kernels that stream rows from memory and have no interpreter op behind them (dsp_extrema.hip, dsp_hist.hip, dsp_thresh.hip)
// a per-event operand: a constant, or a column of the loop's type -- or, now and then, of another
dsp_scalar_arg loop_arg(Prog& p, double lo = 0.0) {
    if (chance(0.5)) return cst(pick({lo, 1.0, 12.5, 100.0, 4000.0}));
    if (chance(0.15)) return sarg(p);
    dsp_scalar_arg a{};
    a.kind = DSP_ARG_INPUT;
    a.index = add_io(p, DSP_IO_SCALAR_IN, chance(0.85) ? p.dtype : pick({DSP_F32, DSP_F64, DSP_I16, DSP_U32}), 1, chance(0.1) ? rnd(0, 3) : 0, pick({1, 1, 1, 0, 2}));
    return a;
}
// LOAD of a fresh slot from rows with a random start and stride: whole 16-byte vectors half of the time
int load_rows(Prog& p, int len, int dtype) {
    const int s = new_slot(p, len);
    const int off = pick({0, 0, 0, 8, 16, 3, rnd(0, 40)}), stride = off + len + pick({0, 0, 0, 8, 16, 1, rnd(0, 40)});
    dsp_op o = op0(DSP_OP_LOAD);
    o.dst = s, o.io = add_io(p, DSP_IO_WF_IN, dtype, len, off, chance(0.05) ? 0 : stride);
    if (chance(0.05)) o.ip[0] = rnd(0, off), o.ip[1] = rnd(0, stride - off - len);
    p.ops.push_back(o);
    return s;
}
int rows_out(Prog& p, int slot) {
    const int off = pick({0, 0, 4, 1});
    dsp_op st = op0(DSP_OP_STORE);
    st.src = slot, st.io = add_io(p, DSP_IO_WF_OUT, chance(0.05) ? DSP_BOOL : p.dtype, p.slots[slot], off, off + p.slots[slot] + pick({0, 0, 4, 3}));
    p.ops.push_back(st);
    return st.io;
}
void store_regs(Prog& p, int first, int n, int dtype) {
    for (int k = 0; k < n; ++k) {
        dsp_op st = op0(DSP_OP_STORE_SCALAR);
        st.io = chance(0.9) ? add_io(p, DSP_IO_SCALAR_OUT, dtype, 1, chance(0.1) ? rnd(0, 3) : 0, pick({1, 1, 2})) : scalar_out(p);
        st.ip[0] = first + k;
        p.ops.push_back(st);
    }
}

// LOAD, MULTI_EXTREMA, STORE of the two lists, STORE_SCALAR of the two counts (match_extrema_shape)
Prog extrema_shape() {
    Prog p;
    p.dtype = chance(0.3) ? DSP_F64 : DSP_F32;
    const int len = some_len(), m = chance(0.9) ? rnd(1, len > 64 ? 64 : (len > 1 ? len - 1 : 1)) : some_len();
    const int s = load_rows(p, len, in_dtype(p)), a = new_slot(p, m), b = new_slot(p, m), r = new_sregs(p, 2);
    dsp_op ex = op0(DSP_OP_MULTI_EXTREMA);
    ex.src = s, ex.dst = a, ex.ip[1] = b, ex.ip[2] = r, ex.ip[0] = pick({0, 0, 1, 3, 3, 2});
    for (int k = 0; k < 4; ++k) ex.sp[k] = loop_arg(p);
    p.ops.push_back(ex);
    const bool swap = chance(0.3);
    rows_out(p, swap ? b : a);
    rows_out(p, chance(0.95) ? (swap ? a : b) : a);
    store_regs(p, r, 2, DSP_U32);
    if (chance(0.2)) std::swap(p.ops[4], p.ops[5]);
    return p;
}

// the three shapes of match_hist_shape: histogram stored; histogram with histogram_stats on its counters; histogram_stats alone
Prog hist_shape() {
    Prog p;
    p.dtype = chance(0.3) ? DSP_F64 : DSP_F32;
    const int m = pick({1, 4, 64, 100, 2048, 2049, rnd(1, 300)}), form = rnd(0, 2);
    if (form == 2) {  // LOAD weights, LOAD edges (either first), HISTOGRAM_STATS, STORE_SCALAR x 3
        const bool edges_first = chance(0.3);
        const int wrong = chance(0.1) ? in_dtype(p) : p.dtype;
        const int x = load_rows(p, edges_first ? m + 1 : m, chance(0.5) ? wrong : p.dtype), y = load_rows(p, edges_first ? m : m + 1, p.dtype), r = new_sregs(p, 3);
        dsp_op st = op0(DSP_OP_HISTOGRAM_STATS);
        st.src = edges_first ? y : x, st.ip[0] = edges_first ? x : y, st.ip[1] = r, st.sp[0] = loop_arg(p);
        p.ops.push_back(st);
        store_regs(p, r, 3, p.dtype);
        return p;
    }
    const int s = load_rows(p, some_len(), in_dtype(p)), w = new_slot(p, m), b = new_slot(p, chance(0.95) ? m + 1 : m);
    dsp_op hi = op0(DSP_OP_HISTOGRAM);
    hi.src = s, hi.dst = w, hi.ip[0] = b, hi.ip[1] = pick({0, 0, 0, 1, 64, 9000, -1});
    p.ops.push_back(hi);
    int r = -1;
    if (form == 1) {
        r = new_sregs(p, 3);
        dsp_op st = op0(DSP_OP_HISTOGRAM_STATS);
        st.src = chance(0.95) ? w : s, st.ip[0] = b, st.ip[1] = r, st.sp[0] = loop_arg(p);
        p.ops.push_back(st);
    }
    if (form == 0 || chance(0.5)) {
        const bool swap = chance(0.3);
        rows_out(p, swap ? b : w);
        rows_out(p, chance(0.95) ? (swap ? w : b) : w);
    }
    if (form == 1) store_regs(p, r, 3, p.dtype);
    return p;
}

// the three shapes of match_thresh_shape: time_over_threshold; multi_time_point_thresh with one list of thresholds, or a list per row
Prog thresh_shape() {
    Prog p;
    p.dtype = chance(0.3) ? DSP_F64 : DSP_F32;
    const int len = some_len(), form = rnd(0, 2);
    if (form == 0) {  // LOAD, TIME_OVER_THRESHOLD, STORE_SCALAR
        const int s = load_rows(p, len, in_dtype(p)), r = new_sregs(p, 1);
        dsp_op o = op0(DSP_OP_TIME_OVER_THRESHOLD);
        o.src = s, o.dst = r, o.sp[0] = loop_arg(p);
        p.ops.push_back(o);
        store_regs(p, r, 1, p.dtype);
        return p;
    }
    const int m = pick({1, 3, 64, 65, rnd(1, 64)});
    const bool lists = form == 2, list_first = lists && chance(0.3);
    int thr = -1;
    if (list_first) thr = load_rows(p, m, chance(0.9) ? p.dtype : in_dtype(p));
    const int s = load_rows(p, len, in_dtype(p));
    if (lists && !list_first) thr = load_rows(p, chance(0.95) ? m : m + 1, chance(0.9) ? p.dtype : in_dtype(p));
    const int t = new_slot(p, m);
    dsp_op o = op0(DSP_OP_MULTI_TIME_POINT_THRESH);
    o.src = s, o.dst = t, o.ip[0] = pick({'i', 'a', 'f', 'b', 'c', 'r', 'n', 'l', 'l', 'z'}), o.ip[1] = lists ? thr : -1;
    if (!lists) o.io = add_io(p, DSP_IO_TAPS, chance(0.95) ? p.dtype : DSP_F32, chance(0.95) ? m : m + 1, pick({0, 0, 2}), 0);
    o.sp[0] = loop_arg(p), o.sp[1] = chance(0.95) ? cst(pick({1.0, -1.0, 2.5, 0.0})) : loop_arg(p);
    p.ops.push_back(o);
    rows_out(p, t);
    return p;
}

void mutate(Prog& p) {
    if (p.ops.empty()) return;
    dsp_op& o = p.ops[rnd(0, (int)p.ops.size() - 1)];
    switch (rnd(0, 7)) {
        case 0: o.dst = wild(); break;
        case 1: o.src = wild(); break;
        case 2: o.io = wild(); break;
        case 3: o.ip[rnd(0, 3)] = wild(); break;
        case 4: o.sp[rnd(0, 3)] = sarg(p); break;
        case 5:
            if (!p.io.empty()) {
                dsp_io_desc& d = p.io[rnd(0, (int)p.io.size() - 1)];
                switch (rnd(0, 3)) {
                    case 0: d.offset = wild(); break;
                    case 1: d.row_stride = wild(); break;
                    case 2: d.len = wild(); break;
                    default: d.dtype = rnd(-1, 8);
                }
            }
            break;
        case 6:
            if (!p.slots.empty()) p.slots[rnd(0, (int)p.slots.size() - 1)] = wild();
            break;
        default: o.opcode = rnd(0, 40);
    }
}

#define REQUIRE(cond, ...)                                             \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "INVARIANT VIOLATED: %s -- ", #cond);     \
            fprintf(stderr, __VA_ARGS__);                              \
            fprintf(stderr, "\n");                                    \
            return false;                                              \
        }                                                              \
    } while (0)

bool check(const Prog& p, const ChainPlan& c) {
    const DevProgram& P = c.host;
    const int ns = (int)p.slots.size();
    const int esz = (c.f64 || c.i64) ? 8 : 4;
    REQUIRE(c.lds_bytes_per_wave == P.lds_elems_per_wave * esz && c.lds_bytes_per_wave <= LDS_BYTES_PER_CU, "LDS %d bytes", c.lds_bytes_per_wave);
    REQUIRE(P.sreg_off + p.n_sregs <= P.scratch_off && P.scratch_off + DSP_SCRATCH_ELEMS <= P.lds_elems_per_wave, "register file / scratch: %d + %d, %d, %d", P.sreg_off,
            p.n_sregs, P.scratch_off, P.lds_elems_per_wave);
    REQUIRE(P.scratch_off % 4 == 0, "scratch alignment %d", P.scratch_off);
    for (int s = 0; s < ns; ++s) {
        const DevSlot& d = P.slots[s];
        REQUIRE(c.slot_base[s] >= 0 && c.slot_base[s] + c.slot_foot[s] <= P.sreg_off, "slot %d region [%d, +%d) beyond the slot area %d", s, c.slot_base[s], c.slot_foot[s], P.sreg_off);
        REQUIRE(c.slot_base[s] % 4 == 0 && c.slot_foot[s] % 4 == 0, "slot %d region alignment", s);
        REQUIRE(d.len == p.slots[s] && d.C % 16 == 0 && d.C * 64 >= d.len && d.pitch == d.C + d.padw && (d.padw == 0 || d.padw == 1), "slot %d geometry len %d C %d pitch %d", s, d.len, d.C, d.pitch);
        REQUIRE(d.off == c.slot_base[s] + 2 * d.pitch && d.off + 64 * d.pitch <= c.slot_base[s] + c.slot_foot[s], "slot %d image outside its region", s);
        REQUIRE(d.zero_below >= 0 && d.zero_below <= 2 * d.pitch && d.zero_above >= 0 && d.off + 64 * d.pitch + d.zero_above <= c.slot_base[s] + c.slot_foot[s], "slot %d zero margins", s);
        for (int t = 0; t < s; ++t) {
            const bool together = c.slot_first_op[s] <= c.slot_last_op[t] && c.slot_first_op[t] <= c.slot_last_op[s];
            const bool overlap = c.slot_base[s] < c.slot_base[t] + c.slot_foot[t] && c.slot_base[t] < c.slot_base[s] + c.slot_foot[s];
            REQUIRE(!(together && overlap), "slots %d and %d are alive together (ops %d..%d, %d..%d) and share LDS", s, t, c.slot_first_op[s], c.slot_last_op[s], c.slot_first_op[t],
                    c.slot_last_op[t]);
            if (overlap) REQUIRE(c.slot_shares[s] && c.slot_shares[t], "slots %d and %d share LDS without the clearing op", s, t);
        }
    }
    if (c.i64) {  // an integer program: the row-per-lane kernel, 8-byte registers, nothing but functions of per-event values and stores
        REQUIRE(c.scalar_ok && ns == 0 && esz == 8, "integer program on %s", dsp_plan_kernel_name(&c));
        for (size_t i = 0; i < p.ops.size(); ++i) REQUIRE(p.ops[i].opcode == DSP_OP_SCALAR_FUNC || p.ops[i].opcode == DSP_OP_STORE_SCALAR, "integer program holds opcode %d", p.ops[i].opcode);
        for (size_t k = 0; k < p.io.size(); ++k)
            if (p.io[k].kind == DSP_IO_SCALAR_IN) REQUIRE(p.io[k].dtype != DSP_F32 && p.io[k].dtype != DSP_F64, "integer program reads a float column");
    } else {
        for (size_t k = 0; k < p.io.size(); ++k)
            if (p.io[k].kind == DSP_IO_SCALAR_OUT || p.io[k].kind == DSP_IO_WF_OUT) REQUIRE(p.io[k].dtype == p.dtype || p.io[k].dtype == DSP_BOOL || (c.kernel_only == DSP_ROUTE_EXTREMA && p.io[k].kind == DSP_IO_SCALAR_OUT && p.io[k].dtype == DSP_U32), "output %zu of type %d in a chain of type %d", k, p.io[k].dtype, p.dtype);
    }
    REQUIRE(P.n_ops >= 1 && P.n_ops <= DSP_MAX_OPS + DSP_MAX_SLOTS, "device ops %d", P.n_ops);
    REQUIRE(P.team >= 1 && P.team <= 3, "team %d", P.team);
    for (int i = 0; i < P.n_ops; ++i) REQUIRE((P.ops[i].member >= 0 && P.ops[i].member < P.team) || P.ops[i].member == DSP_MEMBER_ALL, "op %d member %d", i, P.ops[i].member);
    REQUIRE(c.waves_per_block >= 1 && c.waves_per_block <= 4 && P.waves_per_block == c.waves_per_block, "waves per block %d", c.waves_per_block);
    auto io_ok = [&](int k, int kind) { return k >= 0 && k < (int)p.io.size() && p.io[k].kind == kind; };
    if (c.rr_ok || c.fused_ok) {
        REQUIRE(io_ok(c.io_wf, DSP_IO_WF_IN) && io_ok(c.io_out, DSP_IO_SCALAR_OUT), "energy kernel bindings");
        const EnergyArgs& F = c.rr_ok ? c.rr : c.fused;
        REQUIRE(F.wf_offset == p.io[c.io_wf].offset && F.wf_stride == p.io[c.io_wf].row_stride && F.len == p.io[c.io_wf].len, "energy kernel: the row binding's offset / stride / length");
        REQUIRE((p.io[c.io_wf].offset * dsp_elem_size(p.io[c.io_wf].dtype)) % 16 == 0 && (p.io[c.io_wf].row_stride * dsp_elem_size(p.io[c.io_wf].dtype)) % 16 == 0, "energy kernel on unaligned rows");
        REQUIRE(F.out_stride == p.io[c.io_out].row_stride, "energy kernel: output stride");
        if (c.io_bl >= 0) REQUIRE(io_ok(c.io_bl, DSP_IO_SCALAR_IN) && F.bl_stride == p.io[c.io_bl].row_stride, "energy kernel: baseline column");
        if (c.io_tp >= 0) REQUIRE(io_ok(c.io_tp, DSP_IO_SCALAR_IN) && F.tp_stride == p.io[c.io_tp].row_stride, "energy kernel: pick-off column");
        if (c.rr_ok) REQUIRE(c.rr_lds_bytes > 0 && c.rr_lds_bytes <= LDS_BYTES_PER_CU, "energy kernel LDS %d", c.rr_lds_bytes);
    }
    if (c.rows_ok) {
        REQUIRE(io_ok(c.rio_wf, DSP_IO_WF_IN), "rows kernel: row binding");
        REQUIRE(c.rows.wf_offset == p.io[c.rio_wf].offset && c.rows.wf_stride == p.io[c.rio_wf].row_stride, "rows kernel: the row binding's offset / stride");
        REQUIRE(c.rows.len > 0 && c.rows.len % 8 == 0 && c.rows.len + c.rows.wf_offset <= c.rows.wf_stride, "rows kernel: length %d", c.rows.len);
        REQUIRE(c.rows_lds_bytes > 0 && c.rows_lds_bytes <= LDS_BYTES_PER_CU && c.rows.ring_entries % 8 == 0, "rows kernel LDS %d", c.rows_lds_bytes);
        for (int k = 0; k < 3; ++k) REQUIRE(c.rows.lag[k] >= 8 && c.rows.lag[k] + 8 <= c.rows.ring_entries, "rows kernel: lag %d of a ring of %d", c.rows.lag[k], c.rows.ring_entries);
    }
    if (c.fir_ok) {
        REQUIRE(io_ok(c.fio_wf, DSP_IO_WF_IN), "FIR kernel: row binding");
        REQUIRE(c.fir.wf_offset == p.io[c.fio_wf].offset && c.fir.wf_stride == p.io[c.fio_wf].row_stride && c.fir.n == p.io[c.fio_wf].len, "FIR kernel: the row binding's offset / stride / length");
        REQUIRE(c.fir.n_kernels >= 1 && c.fir.n_kernels <= DSP_FIR_MAXK, "FIR kernels %d", c.fir.n_kernels);
        for (int k = 0; k < c.fir.n_kernels; ++k) {
            REQUIRE(io_ok(c.fio_taps[k], DSP_IO_TAPS) && c.fir.m[k] >= 64 && c.fir.m[k] <= p.io[c.fio_taps[k]].len && c.fir.m[k] <= c.fir.n, "FIR kernel %d: %d taps", k, c.fir.m[k]);
            REQUIRE(c.fio_out[k] >= 0 && c.fio_out[k] < (int)p.io.size(), "FIR kernel %d: output binding", k);
        }
        REQUIRE(c.fir.kend % 32 == 0 && c.fir.kend > 0, "FIR kernel: kend %d", c.fir.kend);
        // (amax form: the staging loads run to the end of the last 32-sample stage, inside the row; kept output: kend is a tile's window)
        if (!c.fir.store) REQUIRE(c.fir.kend + c.fir.wf_offset <= c.fir.wf_stride, "FIR kernel: stages reach %d samples into a row of %lld", c.fir.kend + c.fir.wf_offset, (long long)c.fir.wf_stride);
        REQUIRE(c.fir_lds_bytes > 0 && c.fir_lds_bytes <= LDS_BYTES_PER_CU, "FIR kernel LDS %d", c.fir_lds_bytes);
    }
    if (c.pz_ok) {
        REQUIRE(io_ok(c.pio_wf, DSP_IO_WF_IN) && io_ok(c.pio_out, DSP_IO_WF_OUT), "pole-zero rows: bindings");
        REQUIRE(c.pz.wf_offset == p.io[c.pio_wf].offset && c.pz.wf_stride == p.io[c.pio_wf].row_stride && c.pz.len == p.io[c.pio_wf].len && c.pz.out_stride == p.io[c.pio_out].row_stride,
                "pole-zero rows: the bindings' offset / stride / length");
        REQUIRE(c.pz.len % 8 == 0, "pole-zero rows: length %d", c.pz.len);
        for (int k = 0; k < 4; ++k)
            if (c.pio_mm[k] >= 0) REQUIRE(c.pz.mm_on && io_ok(c.pio_mm[k], DSP_IO_SCALAR_OUT) && c.pz.mm_stride[k] == p.io[c.pio_mm[k]].row_stride, "pole-zero rows: min_max output %d", k);
    }
    if (c.red_ok) {
        REQUIRE(io_ok(c.red_src.io, DSP_IO_WF_IN), "reduce kernel: row binding");
        REQUIRE(c.red.wf_offset == p.io[c.red_src.io].offset && c.red.wf_stride == p.io[c.red_src.io].row_stride && c.red.len == p.io[c.red_src.io].len, "reduce kernel: the row binding's offset / stride / length");
        for (int k = 0; k < DSP_REDUCE_PICKS; ++k)
            if (c.dio_pick[k] >= 0) REQUIRE(c.red.pick_at[k] >= -1 && c.red.pick_at[k] < c.red.len, "reduce kernel: pick-off at %d of %d", c.red.pick_at[k], c.red.len);
        for (int k = 0; k < DSP_REDUCE_WALKS; ++k)
            if (c.dio_walk[k] >= 0 && c.red.walk_from[k] == 0) REQUIRE(c.red.walk_start[k] >= 0 && c.red.walk_start[k] < c.red.len, "reduce kernel: walk from %d of %d", c.red.walk_start[k], c.red.len);
        REQUIRE(c.red.n_walks >= 0 && c.red.n_walks <= DSP_REDUCE_WALKS, "reduce kernel: %d walks", c.red.n_walks);
        for (int k = 0; k < c.red.n_walks; ++k) {
            const int from = c.red.walk_from[k];
            REQUIRE(from >= 0 && from < 4 + k, "reduce kernel: walk %d starts from %d", k, from);
            if (from == 3) REQUIRE(io_ok(c.dio_walk_ts[k], DSP_IO_SCALAR_IN) && p.io[c.dio_walk_ts[k]].dtype == DSP_F32 && c.red.walk_ts_stride[k] == p.io[c.dio_walk_ts[k]].row_stride, "reduce kernel: walk %d's start column", k);
            if (c.red.walk_thr_scaled[k]) REQUIRE(io_ok(c.dio_walk_thr[k], DSP_IO_SCALAR_IN), "reduce kernel: walk %d scales no column", k);
        }
        if (!c.red.need_stream) REQUIRE(c.dio_out[0] < 0 && c.dio_out[4] < 0 && (p.io[c.red_src.io].dtype != DSP_F32 || (p.ops[0].ip[2] & 1)), "reduce kernel: no pass over rows that need one");
    }
    if (c.runs_ok) {
        REQUIRE(!c.red_ok && !c.fir_ok, "run-length FIR beside another kernel of the same program");
        REQUIRE(io_ok(c.uio_wf, DSP_IO_WF_IN) && p.io[c.uio_wf].dtype == DSP_F32 && io_ok(c.uio_taps, DSP_IO_TAPS), "run-length FIR: bindings");
        const FirRunsArgs& R = c.runs;
        REQUIRE(R.wf_offset == p.io[c.uio_wf].offset && R.wf_stride == p.io[c.uio_wf].row_stride && R.n == p.io[c.uio_wf].len, "run-length FIR: the row binding's offset / stride / length");
        REQUIRE(R.n % 8 == 0 && R.wf_offset % 4 == 0 && R.wf_stride % 4 == 0 && R.wf_offset + R.n <= R.wf_stride, "run-length FIR: rows of %d samples at %d of %lld", R.n, R.wf_offset, (long long)R.wf_stride);
        REQUIRE(R.m >= 1 && R.m <= DSP_FIR_RUNS_MAX_TAPS && R.m <= R.n && R.m <= p.io[c.uio_taps].len, "run-length FIR: %d taps", R.m);
        REQUIRE(R.start >= 0 && R.start <= R.m - 1 && R.p >= 1 && R.p + R.start <= R.n + R.m - 1 + R.start && R.p <= R.n + R.m - 1, "run-length FIR: %d outputs from %d", R.p, R.start);
        REQUIRE(R.keep ? (io_ok(c.uio_out, DSP_IO_WF_OUT) && p.io[c.uio_out].len == R.p && R.out_stride == p.io[c.uio_out].row_stride) : (R.has_red && R.out_stride >= R.p),
                "run-length FIR: where the filtered waveform goes");
        if (R.has_red) {
            REQUIRE(R.red.len == R.p, "run-length FIR: reductions over %d of %d outputs", R.red.len, R.p);
            for (int k = 0; k < DSP_REDUCE_PICKS; ++k)
                if (c.dio_pick[k] >= 0) REQUIRE(R.red.pick_at[k] >= -1 && R.red.pick_at[k] < R.p, "run-length FIR: pick-off at %d of %d", R.red.pick_at[k], R.p);
            for (int k = 0; k < DSP_REDUCE_WALKS; ++k)
                if (c.dio_walk[k] >= 0 && R.red.walk_from[k] == 0) REQUIRE(R.red.walk_start[k] >= 0 && R.red.walk_start[k] < R.p, "run-length FIR: walk from %d of %d", R.red.walk_start[k], R.p);
        }
    }
    if (c.cur_ok) {
        REQUIRE(io_ok(c.cio_wf, DSP_IO_WF_IN), "current kernel: row binding");
        REQUIRE(c.cur.wf_offset == p.io[c.cio_wf].offset && c.cur.wf_stride == p.io[c.cio_wf].row_stride && c.cur.n_in == p.io[c.cio_wf].len, "current kernel: the row binding's offset / stride / length");
        REQUIRE(c.cur.win_len < c.cur.n_in && c.cur.n_c == c.cur.win_len - c.cur.ac_lag && c.cur.n_up % 16 == 0 && c.cur.ma_len % 16 == 0 && c.cur.ma_len <= 112 && c.cur.up_shift >= 0 && c.cur.up_shift <= 4,
                "current kernel geometry");
        REQUIRE(c.cur_lds_bytes > 0 && c.cur_lds_bytes <= LDS_BYTES_PER_CU, "current kernel LDS %d", c.cur_lds_bytes);
    }
    // the kernels that stream rows from memory: the row binding, the per-event operands, the outputs
    auto rows_vec = [&](int k) {
        const int64_t es = dsp_elem_size(p.io[k].dtype);
        return (p.io[k].row_stride * es) % 16 == 0 && ((int64_t)p.io[k].offset * es) % 16 == 0 && ((int64_t)p.io[k].len * es) % 16 == 0;
    };
    auto column_ok = [&](int k, int64_t stride) { return io_ok(k, DSP_IO_SCALAR_IN) && p.io[k].dtype == p.dtype && stride == p.io[k].row_stride; };
    auto out_ok = [&](int k, int kind, int64_t stride) { return io_ok(k, kind) && stride == p.io[k].row_stride; };
    // ---- a pretended launch of a kernel-only chain (plan_fuzz_launch.h): every pointer of the block is the one the PROGRAM names -- an
    // output's or a column's first element, an input whose offset travels in the arguments as it is handed in, null what the program has not
    auto first_of = [&](int k) { return ::first_of(p, k); };
    const KernelOnlyArgs launch = c.kernel_only != DSP_ROUTE_VM ? launch_args(p, c) : KernelOnlyArgs{};
    if (c.kernel_only == DSP_ROUTE_EXTREMA) {
        const ExtremaArgs& A = c.only.ext;
        const ExtremaArgs& L = launch.ext;
        const dsp_op& ex = p.ops[1];
        REQUIRE(p.ops.size() == 6 && L.wf == raw_of(p.ops[0].io), "extrema kernel: the rows' pointer");
        for (int k = 0; k < 4; ++k) REQUIRE(L.par[k] == first_of(column_of(ex, k)), "extrema kernel: the pointer of parameter %d", k);
        for (int i = 2; i < 4; ++i) REQUIRE(L.vt_out[p.ops[i].src == ex.dst ? 0 : 1] == first_of(p.ops[i].io), "extrema kernel: the pointer of the list op %d stores", i);
        for (int i = 4; i < 6; ++i) REQUIRE(L.n_out[p.ops[i].ip[0] == ex.ip[2] ? 0 : 1] == first_of(p.ops[i].io), "extrema kernel: the pointer of the count op %d stores", i);
        REQUIRE(io_ok(c.only_src.io, DSP_IO_WF_IN), "extrema kernel: row binding");
        REQUIRE(A.wf_offset == p.io[c.only_src.io].offset && A.wf_stride == p.io[c.only_src.io].row_stride && A.len == p.io[c.only_src.io].len, "extrema kernel: the row binding's offset / stride / length");
        for (int k = 0; k < 4; ++k)
            if (c.bound_io(A.par[k]) >= 0) REQUIRE(column_ok(c.bound_io(A.par[k]), A.par_stride[k]), "extrema kernel: parameter column %d", k);
        for (int k = 0; k < 2; ++k) {
            REQUIRE(out_ok(c.bound_io(A.vt_out[k]), DSP_IO_WF_OUT, A.vt_stride[k]) && p.io[c.bound_io(A.vt_out[k])].len == A.m, "extrema kernel: list %d", k);
            REQUIRE(out_ok(c.bound_io(A.n_out[k]), DSP_IO_SCALAR_OUT, A.n_stride[k]) && p.io[c.bound_io(A.n_out[k])].dtype == DSP_U32, "extrema kernel: count %d", k);
        }
        REQUIRE(A.m >= 1 && A.m < A.len && A.direction >= 0 && A.direction <= 3 && A.direction != 2, "extrema kernel: lists of %d from rows of %d, direction %d", A.m, A.len, A.direction);
        if (c.only_src.vec) REQUIRE(rows_vec(c.only_src.io), "extrema kernel: vector loads on rows that are not whole 16-byte vectors");
    }
    if (c.kernel_only == DSP_ROUTE_HIST) {
        const HistArgs& A = c.only.hist;
        REQUIRE(A.m >= 1 && A.m <= DSP_HIST_MAX_BINS, "histogram kernel: %d bins", A.m);
        const HistArgs& L = launch.hist;
        const bool alone = p.ops[2].opcode == DSP_OP_HISTOGRAM_STATS && p.ops[1].opcode == DSP_OP_LOAD;
        const dsp_op* st = p.ops[2].opcode == DSP_OP_HISTOGRAM_STATS ? &p.ops[2] : nullptr;
        int w_out = -1, b_out = -1, s_out[3] = {-1, -1, -1};
        for (const dsp_op& o : p.ops) {
            if (o.opcode == DSP_OP_STORE) (o.src == p.ops[1].dst ? w_out : b_out) = o.io;
            if (o.opcode == DSP_OP_STORE_SCALAR) s_out[o.ip[0] - st->ip[1]] = o.io;
        }
        if (alone) {
            const dsp_op &lw = p.ops[0].dst == st->src ? p.ops[0] : p.ops[1], &le = p.ops[0].dst == st->ip[0] ? p.ops[0] : p.ops[1];
            REQUIRE(L.wf == nullptr && L.w_in == raw_of(lw.io) && L.e_in == raw_of(le.io), "histogram_stats alone: the pointers of weights and edges");
        } else {
            REQUIRE(L.wf == raw_of(p.ops[0].io) && L.w_in == nullptr && L.e_in == nullptr, "histogram kernel: the rows' pointer");
        }
        REQUIRE(L.w_out == first_of(w_out) && L.b_out == first_of(b_out) && L.max_in == first_of(st ? column_of(*st, 0) : -1), "histogram kernel: the pointers of weights_out, borders_out and max_in");
        for (int k = 0; k < 3; ++k) REQUIRE(L.s_out[k] == first_of(s_out[k]), "histogram kernel: the pointer of histogram_stats output %d", k);
        if (c.only_src.io >= 0) {
            REQUIRE(io_ok(c.only_src.io, DSP_IO_WF_IN), "histogram kernel: row binding");
            REQUIRE(A.wf_offset == p.io[c.only_src.io].offset && A.wf_stride == p.io[c.only_src.io].row_stride && A.len == p.io[c.only_src.io].len, "histogram kernel: the row binding's offset / stride / length");
            REQUIRE(c.bound_io(A.w_in) < 0 && c.bound_io(A.e_in) < 0, "histogram kernel: a row and weights read from memory");
            if (c.only_src.vec) REQUIRE(rows_vec(c.only_src.io), "histogram kernel: vector loads on rows that are not whole 16-byte vectors");
        } else {
            REQUIRE(A.stats && !c.only_src.vec, "histogram kernel: neither a row nor histogram_stats alone");
            REQUIRE(io_ok(c.bound_io(A.w_in), DSP_IO_WF_IN) && p.io[c.bound_io(A.w_in)].dtype == p.dtype && A.w_in_stride == p.io[c.bound_io(A.w_in)].row_stride && A.w_in_offset == p.io[c.bound_io(A.w_in)].offset && p.io[c.bound_io(A.w_in)].len == A.m,
                    "histogram_stats alone: the weights' rows");
            REQUIRE(io_ok(c.bound_io(A.e_in), DSP_IO_WF_IN) && p.io[c.bound_io(A.e_in)].dtype == p.dtype && A.e_in_stride == p.io[c.bound_io(A.e_in)].row_stride && A.e_in_offset == p.io[c.bound_io(A.e_in)].offset && p.io[c.bound_io(A.e_in)].len == A.m + 1,
                    "histogram_stats alone: the edges' rows");
        }
        if (c.bound_io(A.w_out) >= 0 || !A.stats) REQUIRE(out_ok(c.bound_io(A.w_out), DSP_IO_WF_OUT, A.w_stride) && p.io[c.bound_io(A.w_out)].len == A.m, "histogram kernel: weights_out");
        if (c.bound_io(A.b_out) >= 0 || !A.stats) REQUIRE(out_ok(c.bound_io(A.b_out), DSP_IO_WF_OUT, A.b_stride) && p.io[c.bound_io(A.b_out)].len == A.m + 1, "histogram kernel: borders_out");
        if (A.stats) {
            for (int k = 0; k < 3; ++k) REQUIRE(out_ok(c.bound_io(A.s_out[k]), DSP_IO_SCALAR_OUT, A.s_stride[k]), "histogram kernel: histogram_stats output %d", k);
            if (c.bound_io(A.max_in) >= 0) REQUIRE(column_ok(c.bound_io(A.max_in), A.max_in_stride), "histogram kernel: max_in column");
        }
    }
    if (c.kernel_only == DSP_ROUTE_SPECTRUM) {  // (no generator draws psd or fft: main plans two fixed programs ahead of the drawn ones)
        const SpectrumArgs &A = c.only.spec, &L = launch.spec;
        REQUIRE(p.ops.size() == 3 && c.only_src.io == p.ops[0].io && c.bound_io(A.out) == p.ops[2].io, "spectrum kernel: the bindings of rows and output");
        REQUIRE(L.wf == raw_of(p.ops[0].io) && L.out == first_of(p.ops[2].io), "spectrum kernel: the pointers of the rows and the output");
        REQUIRE(L.twiddle == nullptr && L.aux == nullptr && L.filter == nullptr, "spectrum kernel: the tables are the chain's, not the plan's");
    }
    if (c.kernel_only == DSP_ROUTE_THRESH) {
        const ThreshArgs& A = c.only.thresh;
        REQUIRE(io_ok(c.only_src.io, DSP_IO_WF_IN), "threshold kernel: row binding");
        const ThreshArgs& L = launch.thresh;
        const bool lists = p.ops.size() == 4;
        const dsp_op &op = p.ops[lists ? 2 : 1], &store = p.ops.back();
        const dsp_op& ld = !lists || p.ops[0].dst == op.src ? p.ops[0] : p.ops[1];
        REQUIRE(L.wf == raw_of(ld.io) && L.out == first_of(store.io), "threshold kernel: the pointers of the rows and the output");
        if (op.opcode == DSP_OP_TIME_OVER_THRESHOLD) {
            // (as it is handed in: the kernel has always read this column without the binding's offset)
            REQUIRE(L.thr == raw_of(column_of(op, 0)) && L.ts == nullptr, "time_over_threshold: the pointer of the threshold column");
        } else {
            const int thr = lists ? (&ld == &p.ops[0] ? p.ops[1] : p.ops[0]).io : op.io;
            REQUIRE(L.thr == raw_of(thr) && L.ts == first_of(column_of(op, 0)), "multi_time_point_thresh: the pointers of the thresholds and of t_start");
        }
        REQUIRE(A.wf_offset == p.io[c.only_src.io].offset && A.wf_stride == p.io[c.only_src.io].row_stride && A.len == p.io[c.only_src.io].len, "threshold kernel: the row binding's offset / stride / length");
        REQUIRE(A.m >= 0 && A.m <= DSP_THRESH_MAX && A.len >= (A.m > 0 ? 2 : 1), "threshold kernel: %d thresholds on rows of %d", A.m, A.len);
        REQUIRE(out_ok(c.bound_io(A.out), A.m > 0 ? DSP_IO_WF_OUT : DSP_IO_SCALAR_OUT, A.out_stride), "threshold kernel: output");
        if (A.m > 0) {
            REQUIRE((A.polarity == 1 || A.polarity == -1) && strchr("iafbcrnl", A.mode) && p.io[c.bound_io(A.out)].len == A.m, "threshold kernel: polarity %d, mode %d", A.polarity, A.mode);
            REQUIRE(c.bound_io(A.thr) >= 0 && c.bound_io(A.thr) < (int)p.io.size() && p.io[c.bound_io(A.thr)].dtype == p.dtype && p.io[c.bound_io(A.thr)].len == A.m && A.thr_offset == p.io[c.bound_io(A.thr)].offset &&
                        (p.io[c.bound_io(A.thr)].kind == DSP_IO_WF_IN ? A.thr_stride == p.io[c.bound_io(A.thr)].row_stride : (p.io[c.bound_io(A.thr)].kind == DSP_IO_TAPS && A.thr_stride == 0)),
                    "threshold kernel: the thresholds' binding");
            if (c.bound_io(A.ts) >= 0) REQUIRE(column_ok(c.bound_io(A.ts), A.ts_stride), "threshold kernel: t_start column");
        } else {
            REQUIRE(c.bound_io(A.ts) < 0, "time_over_threshold with a t_start");
            if (c.bound_io(A.thr) >= 0) REQUIRE(column_ok(c.bound_io(A.thr), A.thr_stride), "threshold kernel: threshold column");
        }
        if (c.only_src.vec) REQUIRE(rows_vec(c.only_src.io), "threshold kernel: vector loads on rows that are not whole 16-byte vectors");
    }
    return true;
}

void dump(const Prog& p) {
    fprintf(stderr, "program: dtype %d, %zu ops, %zu io, %zu slots, %d sregs\n", p.dtype, p.ops.size(), p.io.size(), p.slots.size(), p.n_sregs);
    for (size_t s = 0; s < p.slots.size(); ++s) fprintf(stderr, "  slot %zu: %d\n", s, p.slots[s]);
    for (size_t k = 0; k < p.io.size(); ++k) fprintf(stderr, "  io %zu: kind %d dtype %d len %d offset %d stride %lld\n", k, p.io[k].kind, p.io[k].dtype, p.io[k].len, p.io[k].offset, (long long)p.io[k].row_stride);
    for (size_t i = 0; i < p.ops.size(); ++i) {
        const dsp_op& o = p.ops[i];
        fprintf(stderr, "  op %zu: opcode %d dst %d src %d io %d ip %d %d %d %d sp", i, o.opcode, o.dst, o.src, o.io, o.ip[0], o.ip[1], o.ip[2], o.ip[3]);
        for (int k = 0; k < 4; ++k) fprintf(stderr, " (%d %d %g)", o.sp[k].kind, o.sp[k].index, o.sp[k].value);
        fprintf(stderr, "\n");
    }
}

// ---- the digest: FNV-1a over named fields (never over a whole argument block: their padding is not defined)
struct Digest {
    uint64_t h = 1469598103934665603ull;
    void bytes(const void* p, size_t n) {
        for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    }
    template <typename T>
    void operator()(const T& v) {
        static_assert(std::is_arithmetic<T>::value, "hash a field, not a structure");
        bytes(&v, sizeof v);
    }
    template <typename T, size_t N>
    void operator()(const T (&a)[N]) {
        for (const T& v : a) (*this)(v);
    }
    void text(const char* s) { bytes(s, strlen(s) + 1); }
};

void digest_reduce(Digest& H, const ReduceArgs& A) {
    H(A.wf_stride), H(A.wf_offset), H(A.len), H(A.out_stride), H(A.pick_stride), H(A.pick_at), H(A.pick_rule), H(A.walk_stride), H(A.walk_thr_stride);
    H(A.walk_thr_const), H(A.walk_from), H(A.walk_start), H(A.walk_forward), H(A.walk_thr_factor), H(A.walk_thr_scaled), H(A.walk_ts_stride), H(A.n_walks), H(A.need_stream);
}

void digest_energy(Digest& H, const EnergyArgs& A) {
    H(A.wf_stride), H(A.wf_offset), H(A.len), H(A.bl_stride), H(A.bl_const), H(A.has_bl), H(A.tp_stride), H(A.tp_const), H(A.mode), H(A.out_stride), H(A.c), H(A.rr), H(A.ll);
    H(A.tau_nan), H(A.all_nan), H(A.C), H(A.pitch), H(A.invC), H(A.q), H(A.rho), H(A.lds_elems_per_wave), H(A.slot_off), H(A.tau_stride), H(A.ablate);
}

void digest_plan(Digest& H, const ChainPlan& c, int n_slots) {
    const DevProgram& P = c.host;
    const bool any_ok = c.scalar_ok || c.pz_ok || c.red_ok || c.runs_ok || c.cur_ok || c.fir_ok || c.rows_ok || c.rr_ok || c.fused_ok;
    H.text(dsp_plan_kernel_name(&c));
    H.text(c.note.c_str());
    H.text(dsp_plan_specialised(&c) ? "" : c.note.c_str());  // (the note as dsp_chain_plan and dsp_chain_kernel_note hand it out)
    H(c.lds_bytes_per_wave), H(c.waves_per_block), H(c.classic_wpb), H(c.has_fir), H(c.f64), H(c.i64);
    H(c.fused_ok), H(c.rr_ok), H(c.rows_ok), H(c.fir_ok), H(c.scalar_ok), H(c.cur_ok), H(c.pz_ok), H(c.red_ok), H(c.runs_ok);
    H((bool)(c.fused_on && any_ok));  // (the switch alone, on a program no kernel takes, shows through no accessor)
    H(c.variant), H(c.fused_trap), H(c.fused_npf), H(c.wf_dtype), H(c.rr_lds_bytes), H(c.rows_lds_bytes), H(c.fir_lds_bytes), H(c.cur_lds_bytes), H(c.fir_f16), H(c.f16.tz);
    H(c.red_src.dtype), H(c.red_src.vec);
    H(c.io_wf), H(c.io_bl), H(c.io_tp), H(c.io_out), H(c.io_tau), H(c.rio_wf), H(c.rio_bl), H(c.rio_thr), H(c.rio_ts), H(c.rio_mm), H(c.rio_tpt), H(c.rio_dwt);
    H(c.fio_wf), H(c.fio_bl), H(c.fio_taps), H(c.fio_out), H(c.cio_wf), H(c.cio_t0), H(c.cio_out), H(c.pio_wf), H(c.pio_bl), H(c.pio_out), H(c.pio_tau), H(c.pio_mm);
    H(c.red_src.io), H(c.dio_out), H(c.dio_pick), H(c.dio_walk), H(c.dio_walk_thr), H(c.dio_walk_ts), H(c.uio_wf), H(c.uio_taps), H(c.uio_out);
    for (int S = 0; S < 2; ++S)
        for (int k = 0; k < 3; ++k) H(c.plan[S].shift[k]), H(c.plan[S].cs[k]), H(c.plan[S].local[k]);
    H(c.slot_base), H(c.slot_foot), H(c.slot_first_op), H(c.slot_last_op), H(c.slot_shares);
    H(P.n_ops), H(P.n_slots), H(P.n_io), H(P.n_sregs), H(P.lds_elems_per_wave), H(P.sreg_off), H(P.waves_per_block), H(P.scratch_off), H(P.team);
    for (int s = 0; s < n_slots; ++s) {
        const DevSlot& d = P.slots[s];
        H(d.off), H(d.len), H(d.C), H(d.pitch), H(d.invC), H(d.padw), H(d.zero_below), H(d.zero_above);
    }
    for (int k = 0; k < P.n_io; ++k) {
        const DevIO& d = P.io[k];
        H(d.kind), H(d.dtype), H(d.len), H(d.offset), H(d.row_stride), H(d.vec_ok);
    }
    H.bytes(P.ops, (size_t)P.n_ops * sizeof(DevOp));  // (every DevOp is cleared before it is filled)
    if (c.fused_ok) digest_energy(H, c.fused);
    if (c.rr_ok) digest_energy(H, c.rr);
    if (c.rows_ok) {
        const RowsArgs& A = c.rows;
        H(A.wf_stride), H(A.wf_offset), H(A.len), H(A.in_kind), H(A.sub_mode), H(A.bl_stride), H(A.bl_const), H(A.pz_kind), H(A.pz_param_nan), H(A.pz_c), H(A.n1), H(A.n2), H(A.d1), H(A.d2);
        H(A.trap_kind), H(A.rise_pow2), H(A.lag), H(A.trap_all_nan), H(A.rr), H(A.ll), H(A.inv_rr), H(A.inv_ll), H(A.out_mm_stride), H(A.tpt_mode), H(A.tpt_use_min), H(A.thr_stride);
        H(A.ts_stride), H(A.thr_const), H(A.ts_const), H(A.walk_nan), H(A.walk_frac), H(A.out_tpt_stride), H(A.dwt_level), H(A.dwt_part), H(A.dwt_stride), H(A.ring_entries), H(A.stop_at_start);
    }
    if (c.fir_ok) {
        const FirArgs& A = c.fir;
        H(A.wf_stride), H(A.wf_offset), H(A.n), H(A.in_kind), H(A.sub_mode), H(A.bl_stride), H(A.bl_const), H(A.n_kernels), H(A.m), H(A.p), H(A.out_stride), H(A.kend), H(A.scan_before);
        H(A.scan_after), H(A.store), H(A.dshift);
    }
    if (c.cur_ok) {
        const CurrentArgs& A = c.cur;
        H(A.wf_stride), H(A.wf_offset), H(A.n_in), H(A.t0_stride), H(A.t0_const), H(A.win_len), H(A.ac_lag), H(A.ac_length), H(A.n_c), H(A.up_shift), H(A.up_half), H(A.n_up), H(A.ma_len);
        H(A.ma_length), H(A.scan_rows), H(A.out_stride), H(A.scratch_per_wave);
    }
    if (c.pz_ok) {
        const PzArgs& A = c.pz;
        H(A.wf_stride), H(A.wf_offset), H(A.len), H(A.in_kind), H(A.sub_mode), H(A.bl_stride), H(A.bl_const), H(A.tau_nan), H(A.c), H(A.out_stride), H(A.tau_stride), H(A.mm_stride), H(A.mm_on);
        H(A.in_lo), H(A.in_hi);
    }
    if (c.red_ok) digest_reduce(H, c.red);
    if (c.runs_ok) {
        const FirRunsArgs& A = c.runs;
        H(A.wf_stride), H(A.wf_offset), H(A.n), H(A.m), H(A.p), H(A.start), H(A.keep), H(A.out_stride), H(A.has_red);
        if (A.has_red) digest_reduce(H, A.red);
    }
    // the kernels that stream rows from memory and have no interpreter op behind them
    // (the values and the order of the members the plan held per route: a route that is not the plan's has no rows and no bindings)
    const RowSource none{};
    auto io = [&](dsp_route route, auto* const& member) { return c.kernel_only == route ? c.bound_io(member) : -1; };
    {
        const ExtremaArgs& A = c.only.ext;
        const RowSource& src = c.kernel_only == DSP_ROUTE_EXTREMA ? c.only_src : none;
        H(c.kernel_only == DSP_ROUTE_EXTREMA), H(src.dtype), H(src.vec), H(src.io);
        for (int k = 0; k < 4; ++k) H(io(DSP_ROUTE_EXTREMA, A.par[k]));
        for (int k = 0; k < 2; ++k) H(io(DSP_ROUTE_EXTREMA, A.vt_out[k]));
        for (int k = 0; k < 2; ++k) H(io(DSP_ROUTE_EXTREMA, A.n_out[k]));
    }
    {
        const HistArgs& A = c.only.hist;
        const RowSource& src = c.kernel_only == DSP_ROUTE_HIST ? c.only_src : none;
        H(c.kernel_only == DSP_ROUTE_HIST), H(src.dtype), H(src.vec), H(src.io);
        H(io(DSP_ROUTE_HIST, A.w_out)), H(io(DSP_ROUTE_HIST, A.b_out)), H(io(DSP_ROUTE_HIST, A.w_in)), H(io(DSP_ROUTE_HIST, A.e_in)), H(io(DSP_ROUTE_HIST, A.max_in));
        for (int k = 0; k < 3; ++k) H(io(DSP_ROUTE_HIST, A.s_out[k]));
    }
    {
        const ThreshArgs& A = c.only.thresh;
        const RowSource& src = c.kernel_only == DSP_ROUTE_THRESH ? c.only_src : none;
        H(c.kernel_only == DSP_ROUTE_THRESH), H(src.dtype), H(src.vec), H(src.io);
        H(io(DSP_ROUTE_THRESH, A.thr)), H(io(DSP_ROUTE_THRESH, A.ts)), H(io(DSP_ROUTE_THRESH, A.out));
    }
    if (c.kernel_only == DSP_ROUTE_EXTREMA) {
        const ExtremaArgs& A = c.only.ext;
        H(A.wf_stride), H(A.wf_offset), H(A.len), H(A.m), H(A.direction), H(A.par_stride), H(A.par_const), H(A.vt_stride), H(A.n_stride);
    }
    if (c.kernel_only == DSP_ROUTE_HIST) {
        const HistArgs& A = c.only.hist;
        H(A.wf_stride), H(A.wf_offset), H(A.len), H(A.m), H(A.stats), H(A.max_blocks), H(A.w_stride), H(A.b_stride), H(A.w_in_stride), H(A.e_in_stride), H(A.w_in_offset), H(A.e_in_offset);
        H(A.max_in_stride), H(A.max_in_const), H(A.s_stride);
    }
    if (c.kernel_only == DSP_ROUTE_THRESH) {
        const ThreshArgs& A = c.only.thresh;
        H(A.wf_stride), H(A.wf_offset), H(A.len), H(A.m), H(A.polarity), H(A.mode), H(A.thr_stride), H(A.thr_offset), H(A.thr_const), H(A.ts_stride), H(A.ts_const), H(A.out_stride);
    }
}

}  // namespace

int main(int argc, char** argv) {
    const long n_programs = argc > 1 ? atol(argv[1]) : 10000;
    const unsigned long long seed = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0xD5BEEDull;
    const bool with_digest = argc > 3 && !strcmp(argv[3], "digest");
    Digest digest;
    rng.seed(seed);
    // the one kernel-only route no generator here or in tests/*_plan_fuzz.cpp draws: psd and fft of rows and spectra that start off their
    // bindings' first element, planned and checked ahead of the drawn programs (no draw is spent, nothing enters the digest)
    for (const int opcode : {DSP_OP_PSD, DSP_OP_FFT}) {
        Prog p;
        const int n = 24, bins = n / 2 + 1, m = opcode == DSP_OP_FFT ? 2 * bins : bins;
        p.slots = {n, m};
        const int in = add_io(p, DSP_IO_WF_IN, DSP_F32, n, 5, n + 9), out = add_io(p, DSP_IO_WF_OUT, DSP_F32, m, 3, m + 3);
        for (const int code : {DSP_OP_LOAD, opcode, DSP_OP_STORE}) p.ops.push_back(op0(code));
        p.ops[0].dst = 0, p.ops[0].io = in, p.ops[1].dst = 1, p.ops[1].src = 0, p.ops[2].src = 1, p.ops[2].io = out;
        ChainPlan plan;
        const int rc = dsp_plan_build(&plan, p.ops.data(), 3, p.io.data(), 2, p.slots.data(), 2, 0, DSP_F32);
        if (rc != DSP_OK || plan.kernel_only != DSP_ROUTE_SPECTRUM || !check(p, plan)) {
            fprintf(stderr, "the fixed %s program: code %d, %s\n", opcode == DSP_OP_PSD ? "psd" : "fft", rc, dsp_plan_last_error());
            return 1;
        }
    }
    long accepted = 0, by_kind[12] = {0}, n_integer = 0;
    long kernels[14] = {0};
    for (long it = 0; it < n_programs; ++it) {
        Prog p;
        const int kind = rnd(0, 20);
        switch (kind) {
            case 0: p = energy_shape(); break;
            case 1: p = rows_shape(); break;
            case 2: p = fir_shape(); break;
            case 3: p = pz_shape(); break;
            case 4: p = reduce_shape(); break;
            case 5: p = current_shape(); break;
            case 6: p = scalar_shape(); break;
            case 7: p = fir_runs_shape(); break;
            case 8: p = extrema_shape(); break;
            case 9: p = hist_shape(); break;
            case 10: p = thresh_shape(); break;
            default: p = random_program();
        }
        if (kind <= 10 && chance(0.3)) mutate(p);
        if (kind > 10 && chance(0.05)) mutate(p);
        if (p.slots.size() > DSP_MAX_SLOTS && chance(0.9)) p.slots.resize(DSP_MAX_SLOTS);
        std::unique_ptr<ChainPlan> plan(new ChainPlan());
        const int rc = dsp_plan_build(plan.get(), p.ops.data(), (int)p.ops.size(), p.io.data(), (int)p.io.size(), p.slots.data(), (int)p.slots.size(), p.n_sregs, p.dtype);
        if (rc != DSP_OK) {
            if (!dsp_plan_last_error()[0] && rc != DSP_E_ZERODIV) {
                fprintf(stderr, "program %ld refused with code %d and no message\n", it, rc);
                dump(p);
                return 1;
            }
            if (with_digest) digest(rc), digest.text(dsp_plan_last_error());
            continue;
        }
        if (with_digest) digest(rc), digest_plan(digest, *plan, (int)p.slots.size());
        ++accepted;
        ++by_kind[kind <= 10 ? kind : 11];
        n_integer += plan->i64 ? 1 : 0;
        switch (dsp_plan_route(plan.get())) {  // (the summary's buckets: the three FIR kernels as one, the interpreter's teams apart)
            case DSP_ROUTE_SCALAR: kernels[0]++; break;
            case DSP_ROUTE_PZ_ROWS: kernels[1]++; break;
            case DSP_ROUTE_REDUCE: kernels[2]++; break;
            case DSP_ROUTE_FIR_RUNS: kernels[10]++; break;
            case DSP_ROUTE_CURRENT: kernels[3]++; break;
            case DSP_ROUTE_FIR_F16: case DSP_ROUTE_FIR_STORE: case DSP_ROUTE_FIR_MFMA: kernels[4]++; break;
            case DSP_ROUTE_ROWS: kernels[5]++; break;
            case DSP_ROUTE_ENERGY_RR: kernels[6]++; break;
            case DSP_ROUTE_ENERGY: kernels[7]++; break;
            case DSP_ROUTE_EXTREMA: kernels[11]++; break;
            case DSP_ROUTE_HIST: kernels[12]++; break;
            case DSP_ROUTE_THRESH: kernels[13]++; break;
            case DSP_ROUTE_VM: kernels[plan->host.team >= 2 ? 8 : 9]++; break;
        }
        if (!check(p, *plan)) {
            fprintf(stderr, "program %ld (seed %llu, kind %d, kernel %s)\n", it, seed, kind, dsp_plan_kernel_name(plan.get()));
            dump(p);
            return 1;
        }
    }
    printf("{\"programs\": %ld, \"accepted\": %ld, \"accepted_by_generator\": {\"energy\": %ld, \"rows\": %ld, \"fir\": %ld, \"pz\": %ld, \"reduce\": %ld, \"current\": %ld, \"scalar\": %ld, \"fir_runs\": %ld, \"extrema\": %ld, \"hist\": %ld, \"thresh\": %ld, \"random\": %ld}, "
           "\"kernels\": {\"scalar\": %ld, \"pz_rows\": %ld, \"reduce\": %ld, \"current\": %ld, \"fir\": %ld, \"rows\": %ld, \"energy_rr\": %ld, \"energy\": %ld, \"vm_team\": %ld, \"vm\": %ld, \"fir_runs\": %ld, \"extrema\": %ld, \"hist\": %ld, \"thresh\": %ld}, \"integer_programs\": %ld",
           n_programs, accepted, by_kind[0], by_kind[1], by_kind[2], by_kind[3], by_kind[4], by_kind[5], by_kind[6], by_kind[7], by_kind[8], by_kind[9], by_kind[10], by_kind[11], kernels[0], kernels[1], kernels[2], kernels[3], kernels[4], kernels[5],
           kernels[6], kernels[7], kernels[8], kernels[9], kernels[10], kernels[11], kernels[12], kernels[13], n_integer);
    if (with_digest) printf(", \"digest\": \"0x%016llx\"", (unsigned long long)digest.h);
    printf("}\n");
    return 0;
}
