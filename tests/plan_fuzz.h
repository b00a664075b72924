// plan_fuzz.h -- what the per-family planner fuzzers (tests/*_plan_fuzz.cpp) share word for word: the generator's draws, a program, the
// REQUIRE of their checks, the plan-or-refuse step of their loops and the addresses of a pretended launch.  What differs on purpose stays in
// the files: wild_length, wild_value, every draw_program and every check.  Each fuzzer is a stand-alone program; this header is all of one
// translation unit with it, so everything here is in the unnamed namespace of that unit.  (The addresses of a pretended launch are
// plan_fuzz_launch.h's, which tests/planner_fuzz.cpp shares: it has a generator, a program and a REQUIRE of its own.)
#pragma once
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

[[maybe_unused]] int32_t clip(int64_t v) { return (int32_t)(v > 0x7fffffff ? 0x7fffffff : v < -0x7fffffff ? -0x7fffffff : v); }
[[maybe_unused]] int64_t times(int64_t a, int64_t b) {  // a product that saturates instead of overflowing
    const __int128 v = (__int128)a * b;
    return v > 0x7fffffff ? 0x7fffffff : v < -0x7fffffff ? -0x7fffffff : (int64_t)v;
}

#define REQUIRE(cond)                                                          \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("program %ld: accepted, but not %s\n", number, #cond); \
            return false;                                                      \
        }                                                                      \
    } while (0)

// The plan of `p`, or null and in *why the reason it is refused with.  A refusal without a reason ends the fuzzer: exit status 1.
std::unique_ptr<ChainPlan> plan_or_refuse(long number, const Prog& p, const char** why) {
    std::unique_ptr<ChainPlan> plan(new ChainPlan());
    const int rc = dsp_plan_build(plan.get(), p.ops.data(), (int)p.ops.size(), p.io.data(), (int)p.io.size(), p.slots.data(), (int)p.slots.size(),
                                  p.n_sregs, p.dtype);
    if (rc == DSP_OK) return plan;
    *why = dsp_plan_last_error();
    if (!*why || !**why) {
        std::printf("program %ld: refused (%d) without a reason\n", number, rc);
        std::exit(1);
    }
    return nullptr;
}

}  // namespace

#include "plan_fuzz_launch.h"
