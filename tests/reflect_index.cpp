// reflect_index.cpp -- the dsp_reflect namespace of dsp_kernels.h (the index rule, the margins, the layout of the staged row and the limits'
// arithmetic of dsp_reflect.hip) on the host, against the processor's formula written out here, for every 1 <= m <= n <= N_MAX.  A
// stand-alone program, built with -fsanitize=address,undefined (tests/test_reflect_index_cpu.py), as tests/interp_index.cpp is for the
// resampling kernel.  The walk of a lane is replayed on an array as long as the LDS a row gets: every read lands inside it, the samples a
// product uses lie inside the staged row, and the sums are the formula's.
//   reflect_index     prints {"pairs": .., "outputs": .., "products": .., "failures": ..}
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../dspeed_amd/csrc/dsp_kernels.h"

namespace {

constexpr int N_MAX = 70;
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

// the formula: out[i] = sum_k kernel[k] * w[r(i + (m-1)//2 - k)], r(t) = -t below 0, 2 (n - 1) - t above n - 1
int formula_source(int i, int k, int n, int m) {
    const int t = i + (m - 1) / 2 - k;
    return t < 0 ? -t : (t > n - 1 ? 2 * (n - 1) - t : t);
}

long check_pair(int n, int m, int esz, long* products) {
    using namespace dsp_reflect;
    const int V = vec(esz), P = pad(m, esz), M = m + P, E = elems(n, m, esz);
    EXPECT(left(m) + right(m) + 1 == m && centre(m) == right(m), "n %d m %d", n, m);
    EXPECT(M % V == 0 && P >= 0 && P < V && E % V == 0 && E >= P + staged(n, m), "n %d m %d esz %d", n, m, esz);
    EXPECT(row_bytes(n, m, esz) == E * esz && lds_bytes(n, m, esz) == (wide(n, m, esz) ? E * esz + 16 : 4 * E * esz), "n %d m %d", n, m);
    // the staged row: position P + j holds sample source(j); the staging pass writes a sample at its own place and at its mirror images
    std::vector<long> lds((size_t)E, -1);  // -1: never written
    for (int at = 0; at < n; ++at) {
        lds[(size_t)(P + left(m) + at)] = at;
        if (at >= 1 && at <= left(m)) lds[(size_t)(P + left(m) - at)] = at;
        if (at >= n - 1 - right(m) && at <= n - 2) lds[(size_t)(P + left(m) + 2 * (n - 1) - at)] = at;
    }
    for (int j = 0; j < staged(n, m); ++j) {
        EXPECT(source(j, n, m) >= 0 && source(j, n, m) < n, "n %d m %d j %d", n, m, j);
        EXPECT(lds[(size_t)(P + j)] == source(j, n, m), "n %d m %d j %d: staged %ld, rule %d", n, m, j, lds[(size_t)(P + j)], source(j, n, m));
    }
    // a lane's walk: V outputs from i0, the taps V a step from tap 0; the vector of a step starts at i0 + M - k0 - V
    long outputs = 0;
    for (int i0 = 0; i0 < n; i0 += V) {
        EXPECT(i0 + M + V <= E, "the first vector of the run at %d ends at %d of %d (n %d m %d)", i0, i0 + M + V, E, n, m);
        for (int k0 = 0; k0 < m; k0 += V) {
            const int lo = i0 + M - k0 - V;
            EXPECT(lo >= 0 && lo % V == 0 && lo + 2 * V <= E, "n %d m %d i0 %d k0 %d: vector at %d", n, m, i0, k0, lo);
            for (int t = 0; t < V && k0 + t < m; ++t)
                for (int r = 0; r < V && i0 + r < n; ++r) {
                    const int at = lo + V - 1 - t + r;  // win[V - 1 - t + r]
                    EXPECT(at >= P && at < P + staged(n, m), "n %d m %d: a product reads position %d outside the staged row", n, m, at);
                    EXPECT(lds[(size_t)at] == formula_source(i0 + r, k0 + t, n, m), "n %d m %d output %d tap %d: sample %ld, the formula's %d", n, m, i0 + r, k0 + t,
                           lds[(size_t)at], formula_source(i0 + r, k0 + t, n, m));
                    ++*products;
                }
        }
        outputs += i0 + V <= n ? V : n - i0;
    }
    // the fused avg_current writes output i to position i: below everything the outputs above it read
    for (int i0 = 0; i0 < n; i0 += V) EXPECT(i0 + M - (m - 1) / V * V - V == i0, "n %d m %d: the lowest vector of the run at %d", n, m, i0);
    return outputs;
}

}  // namespace

int main() {
    using namespace dsp_reflect;
    long pairs = 0, outputs = 0, products = 0;
    for (int n = 1; n <= N_MAX; ++n)
        for (int m = 1; m <= n; ++m) {
            for (int t = -(m / 2); t <= n - 1 + (m - 1) / 2; ++t) EXPECT(reflect(t, n) >= 0 && reflect(t, n) < n, "n %d m %d t %d", n, m, t);
            outputs += check_pair(n, m, 4, &products);
            check_pair(n, m, 8, &products);
            ++pairs;
        }
    // the limits' arithmetic: what fits is what the planner admits, the narrow geometry holds four rows in the LDS of one wide row's worth,
    // and the longest rows stay within 32 bytes + the flag word of 64 KiB
    for (int esz : {4, 8}) {
        const int lim = max_staged(esz);
        EXPECT(lim * esz == LDS_MAX, "esz %d", esz);
        for (int m : {1, 2, 3, 4, 5, 9, 257, 4096, lim / 2, lim / 2 + 1}) {
            const int n = lim + 1 - m;  // n + m - 1 == lim
            if (m > n) continue;
            EXPECT(fits(n, m, esz) && !fits(n + 1, m, esz) && (m + 1 > n || !fits(n, m + 1, esz)), "esz %d m %d", esz, m);
            EXPECT(wide(n, m, esz) && lds_bytes(n, m, esz) <= LDS_MAX + 32 + 16, "esz %d m %d: %d bytes", esz, m, lds_bytes(n, m, esz));
        }
        const int edge = WAVE_ROW_BYTES / esz;
        for (int m : {1, 2, 9, 64}) {
            const int n = edge + 1 - m;
            EXPECT(!wide(n, m, esz) && wide(n + 1, m, esz) && lds_bytes(n, m, esz) <= 4 * (WAVE_ROW_BYTES + 32), "esz %d m %d", esz, m);
        }
        EXPECT(!fits(0x7fffffff, 0x7fffffff, esz) && !fits(0x7fffffff, 1, esz), "no overflow at the largest lengths");
    }
    std::printf("{\"pairs\": %ld, \"outputs\": %ld, \"products\": %ld, \"failures\": %ld}\n", pairs, outputs, products, failures);
    return failures ? 1 : 0;
}
