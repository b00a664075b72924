// sort_network.cpp -- the schedule of dsp_sort.hip (dsp_kernels.h, namespace dsp_sort) on the CPU: the key map, the padding, every step's
// partner, direction and kind, in the order the schedule lists them and in the order the kernel's passes run them.  A stand-alone program
// (tests/test_sort_network_cpu.py builds it with -fsanitize=address,undefined): for every length the result must equal std::sort of the
// keys.  Prints one line of counts and returns 0, or says what failed and returns 1.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../dspeed_amd/csrc/dsp_kernels.h"

using namespace dsp_sort;

static int failures = 0;
#define CHECK(cond, ...)                   \
    do {                                   \
        if (!(cond)) {                     \
            if (failures++ < 20) {         \
                std::printf("FAILED %s: ", #cond); \
                std::printf(__VA_ARGS__);  \
                std::printf("\n");         \
            }                              \
        }                                  \
    } while (0)

template <typename F>
struct Bits;
template <>
struct Bits<float> {
    typedef uint32_t U;
    static constexpr U POS_INF = KEY_POS_INF32, NEG_INF = KEY_NEG_INF32;
};
template <>
struct Bits<double> {
    typedef uint64_t U;
    static constexpr U POS_INF = KEY_POS_INF64, NEG_INF = KEY_NEG_INF64;
};
template <typename F>
typename Bits<F>::U bits(F v) {
    typename Bits<F>::U b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static uint64_t lcg() {
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return lcg_state >> 11;
}

// the row families of tests/sort_cases.py, without the NaN rows (a row with a NaN is never sorted)
template <typename F>
std::vector<F> family(int which, int n) {
    const F inf = std::numeric_limits<F>::infinity(), tiny = std::numeric_limits<F>::denorm_min();
    std::vector<F> w(n);
    for (int i = 0; i < n; ++i) {
        const double u = (double)(lcg() % 2000001) / 1000000.0 - 1.0;  // [-1, 1]
        switch (which) {
            case 0: w[i] = (F)i; break;                       // sorted
            case 1: w[i] = (F)(n - i); break;                 // reversed
            case 2: w[i] = (F)7.25; break;                    // all equal
            case 3: w[i] = (i & 1) ? (F)-3 : (F)5; break;     // two values
            case 4: w[i] = (F)(int)(lcg() % 9) - (F)4; break; // small integers, many duplicates
            case 5: w[i] = (lcg() % 8 == 0) ? (F)((lcg() & 1) ? 1 : -1) * tiny * (F)(lcg() % 5) : (F)(u * 1e3); break;  // mixed sign, denormals
            case 6: w[i] = (lcg() % 5 == 0) ? ((lcg() & 1) ? inf : -inf) : (F)u; break;  // infinities
            case 7: w[i] = (lcg() % 3 == 0) ? ((lcg() & 1) ? (F)0.0 : (F)-0.0) : (F)u; break;  // both zeros
            default: w[i] = (i % 3 == 0) ? inf : (F)u; break;  // +inf samples, which tie with the padding
        }
    }
    return w;
}
constexpr int FAMILIES = 9;

template <typename U>
void exchange(std::vector<U>& key, int i, int k, int j) {
    const int p = partner(i, j);
    if (p < i) return;  // (the pair is the lower index's)
    const U lo = std::min(key[i], key[p]), hi = std::max(key[i], key[p]);
    key[i] = keeps_min(i, k, j) ? lo : hi;
    key[p] = keeps_min(p, k, j) ? lo : hi;
}

// every step of the schedule in order, on all keys
template <typename U>
void run_schedule(std::vector<U>& key, int P) {
    for (int s = 0; s < steps(P); ++s) {
        const Step st = step(P, s);
        for (int i = 0; i < P; ++i) exchange(key, i, st.k, st.j);
    }
}

// the kernel's order: a tile pass runs the steps below TILE of stages k_lo .. k_hi tile after tile, an LDS step runs on all keys.
// Returns the passes over the row.
template <typename U>
int run_passes(std::vector<U>& key, int P) {
    int passes = 0;
    auto tile_pass = [&](int k_lo, int k_hi) {
        for (int t0 = 0; t0 < P; t0 += TILE)
            for (int k = k_lo; k <= k_hi; k <<= 1)
                for (int j = std::min(k >> 1, TILE >> 1); j >= 1; j >>= 1) {
                    CHECK(kind(j) != LDS, "stride %d in a tile pass", j);
                    for (int i = t0; i < std::min(t0 + TILE, P); ++i) exchange(key, i, k, j);
                }
        ++passes;
    };
    tile_pass(2, std::min(P, TILE));
    for (int k = 2 * TILE; k <= P; k <<= 1) {
        for (int j = k >> 1; j >= TILE; j >>= 1) {
            CHECK(kind(j) == LDS, "stride %d as an LDS step", j);
            for (int t = 0; t < P / 2; ++t) {  // (the kernel's pair index -> the lower key of the pair)
                const int low = t & (j - 1), i = ((t - low) << 1) | low;
                CHECK(i >= 0 && i + j < P && (i & j) == 0, "pair %d of stride %d: keys %d and %d of %d", t, j, i, i + j, P);
                exchange(key, i, k, j);
            }
            ++passes;
        }
        tile_pass(k, k);
    }
    return passes;
}

static long steps_seen = 0, rows_sorted = 0;

static void check_schedule(int P) {
    CHECK(P >= CHUNK && (P & (P - 1)) == 0, "P = %d", P);
    int expect_k = 2, expect_j = 1;
    for (int s = 0; s < steps(P); ++s, ++steps_seen) {
        const Step st = step(P, s);
        CHECK(st.k == expect_k && st.j == expect_j, "step %d of %d: (%d, %d), expected (%d, %d)", s, P, st.k, st.j, expect_k, expect_j);
        if (expect_j == 1) expect_k *= 2, expect_j = expect_k / 2; else expect_j /= 2;
        // the kind says where the two keys of every pair meet: exactly one of a lane's chunk, a wavefront's tile, LDS
        int in_chunk = 0, in_tile = 0, apart = 0;
        for (int i = 0; i < P; ++i) {
            const int p = partner(i, st.j);
            CHECK(p >= 0 && p < P && p != i && partner(p, st.j) == i, "partner %d of %d at stride %d, P %d", p, i, st.j, P);
            CHECK(keeps_min(i, st.k, st.j) != keeps_min(p, st.k, st.j), "both ends of pair %d, %d keep the same", i, p);
            CHECK(ascends(i, st.k) == ascends(p, st.k), "pair %d, %d in two runs", i, p);
            if (i / CHUNK == p / CHUNK) ++in_chunk;
            else if (i / TILE == p / TILE) ++in_tile;
            else ++apart;
        }
        const Kind kd = kind(st.j);
        CHECK((in_chunk == P) + (in_tile == P) + (apart == P) == 1, "stride %d mixes kinds", st.j);
        CHECK(kd == (in_chunk == P ? REGISTER : in_tile == P ? CROSS_LANE : LDS), "stride %d is kind %d", st.j, (int)kd);
    }
    CHECK(expect_k == 2 * P, "the last stage of %d is %d", P, expect_k / 2);
}

template <typename F>
void check_length(int n) {
    typedef typename Bits<F>::U U;
    const int P = padded(n);
    CHECK(P >= n && P >= CHUNK && (P == CHUNK || P / 2 < n), "padded(%d) = %d", n, P);
    for (int f = 0; f < FAMILIES; ++f) {
        const std::vector<F> w = family<F>(f, n);
        std::vector<U> key(P, Bits<F>::POS_INF);
        for (int i = 0; i < n; ++i) {
            key[i] = key_of(bits(w[i]));
            CHECK(!key_is_nan(key[i]) && bits_of(key[i]) == bits(w[i]), "key of sample %d, family %d", i, f);
        }
        std::vector<U> want(key.begin(), key.begin() + n);
        std::sort(want.begin(), want.end());
        std::vector<U> a = key, b = key;
        run_schedule(a, P);
        const int passes = run_passes(b, P);
        CHECK(passes == lds_passes(P), "%d passes over %d keys, lds_passes says %d", passes, P, lds_passes(P));
        CHECK(std::equal(want.begin(), want.end(), a.begin()), "schedule order, n %d family %d", n, f);
        CHECK(std::equal(want.begin(), want.end(), b.begin()), "pass order, n %d family %d", n, f);
        for (int i = n; i < P; ++i) CHECK(a[i] == Bits<F>::POS_INF && b[i] == Bits<F>::POS_INF, "padding at %d of %d", i, P);
        // the order of the keys is the order of the values (and -0.0 comes before +0.0)
        for (int i = 1; i < n; ++i) {
            F x, y;
            const U bx = bits_of(a[i - 1]), by = bits_of(a[i]);
            std::memcpy(&x, &bx, sizeof x);
            std::memcpy(&y, &by, sizeof y);
            CHECK(x <= y && !(x == y && std::signbit(y) && !std::signbit(x)), "values at %d, n %d family %d", i, n, f);
        }
        ++rows_sorted;
    }
}

template <typename F>
void check_keys() {
    typedef typename Bits<F>::U U;
    const F inf = std::numeric_limits<F>::infinity();
    CHECK(key_of(bits(-inf)) == Bits<F>::NEG_INF && key_of(bits(inf)) == Bits<F>::POS_INF, "keys of the infinities");
    CHECK(key_of(bits((F)-0.0)) + 1 == key_of(bits((F)0.0)), "the zeros are neighbours");
    const int mant = sizeof(F) == 4 ? 23 : 52;
    const U exp_all = bits(inf);
    for (U sign : {(U)0, (U)1 << (8 * sizeof(U) - 1)})
        for (U payload : {(U)1, (U)1 << (mant - 1), ((U)1 << mant) - 1, ((U)1 << (mant - 1)) + 5})
            CHECK(key_is_nan(key_of((U)(sign | exp_all | payload))), "a NaN's key");
    for (F v : {(F)0.0, (F)-0.0, (F)1, (F)-1, std::numeric_limits<F>::max(), std::numeric_limits<F>::lowest(), std::numeric_limits<F>::denorm_min(), inf, -inf})
        CHECK(!key_is_nan(key_of(bits(v))), "a number's key");
}

int main() {
    check_keys<float>();
    check_keys<double>();
    static_assert(padded(1) == CHUNK && padded(8) == 8 && padded(9) == 16 && padded(16384) == 16384 && padded(16383) == 16384, "padded");
    static_assert(!wide(NARROW_MAX) && wide(NARROW_MAX + 1), "the geometry's threshold");
    static_assert(lds_bytes(16384, 4) == 64 * 1024 + 16 && lds_bytes(8192, 8) == 64 * 1024 + 16 && lds_bytes(NARROW_MAX, 8) == 64 * 1024, "LDS");
    static_assert(lds_passes(1024) == 3 && lds_passes(8192) == 15 && lds_passes(512) == 1 && lds_passes(8) == 1, "passes");
    for (int P = CHUNK; P <= 16384; P *= 2) check_schedule(P);
    std::vector<int> lengths;
    for (int n = 1; n <= 300; ++n) lengths.push_back(n);
    for (int n : {511, 512, 513, 1000, 1023, 1024, 1025, NARROW_MAX - 1, NARROW_MAX, NARROW_MAX + 1, 4095, 4096, 4097, 8192, 16383, 16384}) lengths.push_back(n);
    for (int n : lengths) {
        check_length<float>(n);
        if (n <= 8192) check_length<double>(n);
    }
    std::printf("{\"steps\": %ld, \"rows\": %ld, \"failures\": %d}\n", steps_seen, rows_sorted, failures);
    return failures ? 1 : 0;
}
