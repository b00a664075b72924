// plan_fuzz_launch.h -- a pretended launch of an accepted kernel-only program, for the planner fuzzers (tests/plan_fuzz.h and
// tests/planner_fuzz.cpp, whose `Program`s both hold the bindings as `io`): the block dsp_internal_plan_fill_args makes from addresses
// nobody dereferences, and the pointers that block must hold as the PROGRAM names them.
#pragma once
#include <vector>

#include "../dspeed_amd/csrc/dsp_plan.h"

namespace {

// Binding k lies at an address nobody dereferences; the addresses are 16-byte aligned and 2^40 bytes apart, wider than any offset (below 2^31
// elements of at most 8 bytes).
void* base_of(int io) { return io < 0 ? nullptr : (void*)((uintptr_t)(io + 1) << 40); }
// what the launch hands the kernel (dsp_internal_plan_fill_args): the plan's block, its pointers those of this call
template <typename Program>
KernelOnlyArgs launch_args(const Program& p, const ChainPlan& c) {
    std::vector<void*> io_ptrs;
    for (int k = 0; k < (int)p.io.size(); ++k) io_ptrs.push_back(base_of(k));
    KernelOnlyArgs args;
    dsp_internal_plan_fill_args(&c, io_ptrs.data(), &args);
    return args;
}
// The pointers a block must hold, from the PROGRAM: an output's or a column's first element -- null where the program has none (io < 0) --
// and an input whose offset travels in the arguments as it is handed in
template <typename Program>
const void* first_of(const Program& p, int io) { return io < 0 ? nullptr : (const char*)base_of(io) + (int64_t)p.io[io].offset * dsp_elem_size(p.io[io].dtype); }
const void* raw_of(int io) { return base_of(io); }
// the column operand k of `o` holds, or -1: a constant
int column_of(const dsp_op& o, int k) { return o.sp[k].kind == DSP_ARG_INPUT ? o.sp[k].index : -1; }
// a kernel's 16-byte stores: on where the output is there, starts on a vector and has a stride of whole vectors
template <typename Program>
int vector_store(const Program& p, int io, int loop_esz) {
    if (io < 0) return 0;
    const int64_t es = dsp_elem_size(p.io[io].dtype);
    return (p.io[io].row_stride * loop_esz) % 16 == 0 && (p.io[io].offset * es) % 16 == 0 ? 1 : 0;
}

}  // namespace
