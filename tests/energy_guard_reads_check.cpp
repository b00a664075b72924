// energy_guard_reads_check.cpp -- where the lanes of the register-resident energy kernel read their lagged streams (lag_window_start in
// dsp_kernels.h, which the kernel calls) and the LDS region those reads have to stay in (layout), checked by brute force on the CPU:
// every lane, every lag from 1 to 64 C + 200, at the four chunk lengths the kernel is built for.  Built and run by
// tests/test_energy_guard_reads_cpu.py; prints one JSON line.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "dsp_kernels.h"

using namespace dsp_energy_rr;

#define REQUIRE(cond, ...)                     \
    do {                                       \
        if (!(cond)) {                         \
            std::fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");        \
            std::exit(1);                      \
        }                                      \
    } while (0)

static_assert(lag_window_start(66, layout(66).guard, 0, 625) % 2 == 0, "usable in constant expressions");

int main() {
    const int LDS_BYTES_PER_CU = 160 * 1024;
    long windows = 0, redirected = 0, moved = 0;
    for (int C : {18, 34, 66, 130}) {
        const Layout L = layout(C);
        const int ng1 = (C - 2) / 8 + 1;
        // ---- the region: guard, image, tail, side arrays, capture buffer
        REQUIRE(L.guard >= 2 * C + 8 && L.guard >= C + 64 + WINDOW_SPAN_EXTRA && L.guard % 2 == 0, "guard %d at C = %d", L.guard, C);
        REQUIRE(L.slot_off >= L.guard && L.slot_off % 4 == 0 && L.slot_off < L.guard + 4, "slot_off %d, guard %d", L.slot_off, L.guard);
        REQUIRE(L.tail >= WINDOW_SPAN_EXTRA && L.side_pitch % 2 == 1 && L.side_pitch >= ng1, "tail %d, side pitch %d at C = %d", L.tail, L.side_pitch, C);
        REQUIRE(L.elems % 4 == 0 && L.elems >= L.slot_off + 64 * C + L.tail + 64 * L.side_pitch + 32, "%d elements at C = %d", L.elems, C);
        // wavefronts of a compute unit: 8 (two per SIMD) up to 4096 samples, 4 at 8192 (one per SIMD: its 130 samples a lane fill the registers)
        const int waves = C <= 66 ? 8 : 4;
        REQUIRE(waves * L.elems * 4 <= LDS_BYTES_PER_CU, "%d wavefronts x %d bytes at C = %d", waves, L.elems * 4, C);
        const int span = C + WINDOW_SPAN_EXTRA;  // elements a lane can touch from its window's start
        for (int lag = 1; lag <= 64 * C + 200; ++lag) {
            int start[64];
            for (int lane = 0; lane < 64; ++lane) {
                const int natural = lane * C - lag - (lag & 1), first = lane * C - lag;  // first sample of the window; its last is first + C - 1
                const int s = start[lane] = lag_window_start(C, L.guard, lane, lag);
                ++windows;
                REQUIRE(s % 2 == 0, "odd start %d (C %d lane %d lag %d)", s, C, lane, lag);
                if (first + C - 1 < 0) {  // wholly below sample 0: zeros from the guard, every pair of them, at the natural address modulo 64 elements
                    ++redirected;
                    moved += s != natural;
                    REQUIRE(s >= -L.guard && s + span <= 0, "start %d, span %d, guard %d (C %d lane %d lag %d)", s, span, L.guard, C, lane, lag);
                    REQUIRE(((s - natural) % 64) == 0, "start %d, natural %d (C %d lane %d lag %d)", s, natural, C, lane, lag);
                } else {  // a sample >= 0 in the window: the true address, inside guard + image + tail
                    REQUIRE(s == natural, "start %d, natural %d (C %d lane %d lag %d)", s, natural, C, lane, lag);
                    REQUIRE(s >= -L.guard && s + span <= 64 * C + L.tail, "start %d (C %d lane %d lag %d)", s, C, lane, lag);
                }
            }
            // an 8-byte read of 32 lanes is served by 64 banks: the 32 pairs must differ modulo 32 pairs, in both halves of the wavefront
            for (int half = 0; half < 2; ++half) {
                unsigned seen = 0;
                for (int lane = 32 * half; lane < 32 * half + 32; ++lane) {
                    const int pair = (((start[lane] / 2) % 32) + 32) % 32;
                    REQUIRE(!((seen >> pair) & 1u), "two lanes on pair %d (C %d half %d lag %d)", pair, C, half, lag);
                    seen |= 1u << pair;
                }
            }
        }
    }
    std::printf("{\"windows\": %ld, \"redirected\": %ld, \"moved\": %ld}\n", windows, redirected, moved);
    return 0;
}
