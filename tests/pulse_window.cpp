// pulse_window.cpp -- the dsp_pulses namespace of dsp_kernels.h (the window of a candidate, the dropped candidates and the clamped width of
// dsp_pulses.hip, which the planner uses too) on the host, against the processor's loop written out here, for every row length, candidate
// and width up to small limits.  A stand-alone program, built with -fsanitize=address,undefined (tests/test_pulse_window_cpu.py), as
// tests/reflect_index.cpp is for the mirrored FIR.  A lane's walk is replayed on an array exactly as long as the row: every read lands
// inside it, and the minimum it finds is the brute-force loop's, index for index.
//   pulse_window     prints {"triples": .., "reads": .., "dropped": .., "failures": ..}
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../dspeed_amd/csrc/dsp_kernels.h"

namespace {

constexpr int N_MAX = 40, WIDTH_MAX = 45;
long failures = 0;

#define EXPECT(cond, ...)                           \
    do {                                            \
        if (!(cond)) {                              \
            if (++failures < 20) {                  \
                std::printf("not %s: ", #cond);     \
                std::printf(__VA_ARGS__);           \
                std::printf("\n");                  \
            }                                       \
        }                                           \
    } while (0)

// peak_snr_threshold.py:58-67 for a candidate with int(idx) = c: the bounds, then the search
void brute(const std::vector<double>& w, int c, int width, int* a_out, int* b_out, int* min_index) {
    const int n = (int)w.size();
    int a = c - width, b = c + width;
    if (a < 0) a = 0;
    if (b >= n) b = n - 1;
    int lowest = a;
    for (int j = a; j < b; ++j)
        if (w.at((size_t)j) < w.at((size_t)lowest)) lowest = j;
    *a_out = a, *b_out = b, *min_index = lowest;
}

}  // namespace

int main() {
    using namespace dsp_pulses;
    long triples = 0, reads = 0, n_dropped = 0;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (int n = 1; n <= N_MAX; ++n) {
        std::vector<double> w((size_t)n);
        for (int j = 0; j < n; ++j) w[(size_t)j] = (double)((j * 7 + n) % 5);  // ties everywhere
        // the candidates no sample is read for
        for (double idx : {nan, inf, -inf, -1.0, -1.5, -1e30, (double)n, (double)n + 0.5, 1e30, 4294967296.0 + 3}) {
            EXPECT(dropped(idx, n), "n %d idx %g", n, idx);
            ++n_dropped;
        }
        for (double frac : {0.0, 0.25, 0.5, 0.999}) {
            for (int c = 0; c < n; ++c) {
                const double idx = (double)c + frac;
                if (idx >= (double)n) continue;
                EXPECT(!dropped(idx, n), "n %d idx %g", n, idx);
                for (int width = 0; width <= WIDTH_MAX; ++width) {
                    const Window win = window(idx, n, clamped_width((double)width + frac, n));  // (int(width_in) cuts the fraction)
                    int a, b, want;
                    brute(w, c, width, &a, &b, &want);
                    EXPECT(win.c == c && win.a == a && win.b == b, "n %d c %d width %d: window (%d, %d, %d), the loop's (%d, %d, %d)", n, c, width, win.c, win.a, win.b, c, a, b);
                    EXPECT(win.a >= 0 && win.a <= win.c && win.c < n && win.b <= n - 1 && win.b >= win.a, "n %d c %d width %d", n, c, width);
                    // the lane's walk: strict comparison from w[a], ascending j in [a, b)
                    int lowest = win.a;
                    double low = w.at((size_t)win.a);
                    ++reads;
                    for (int j = win.a; j < win.b; ++j, ++reads)
                        if (w.at((size_t)j) < low) low = w.at((size_t)j), lowest = j;
                    EXPECT(lowest == want, "n %d c %d width %d: min_index %d, the loop's %d", n, c, width, lowest, want);
                    ++triples;
                }
            }
            // a negative fraction in (-1, 0) truncates to 0
            if (frac > 0.0) {
                EXPECT(!dropped(-frac, n) && window(-frac, n, 1).c == 0 && window(-frac, n, 1).a == 0, "n %d idx %g", n, -frac);
            }
        }
        // widths beyond the row, and beyond int
        for (double wide : {(double)n, (double)n + 7, 1e9, 3e9, 1e300, inf}) {
            EXPECT(clamped_width(wide, n) == n, "n %d width %g", n, wide);
            const Window win = window((double)(n - 1), n, clamped_width(wide, n));
            EXPECT(win.a == 0 && win.b == n - 1, "n %d width %g", n, wide);
        }
    }
    // no overflow at the largest lengths
    const int big = 0x7fffffff;
    const Window win = window((double)(big - 1), big, clamped_width(1e18, big));
    EXPECT(win.c == big - 1 && win.a == 0 && win.b == big - 1 && !dropped((double)(big - 1), big) && dropped((double)big, big), "the largest row");
    std::printf("{\"triples\": %ld, \"reads\": %ld, \"dropped\": %ld, \"failures\": %ld}\n", triples, reads, n_dropped, failures);
    return failures ? 1 : 0;
}
