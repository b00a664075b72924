// interp_index.cpp -- the index rules of dsp_interp.hip (dsp_kernels.h, dsp_interp) against the reference's loops run forward.  A stand-alone
// program, built with -fsanitize=address,undefined (tests/test_interp_index_cpu.py); no HIP.
//
// The reference (processors/upsampler.py:112-213) walks the input samples and fills intervals of outputs; restated here as those loops, in
// C++, writing for every output the input segment that wrote it LAST and what kind of value it got.  The kernel walks the outputs:
// dsp_interp::map(mode, n, m, o), and along a lane's consecutive outputs locate() once and advance() after it.  For every n <= 130,
// m <= 400 and mode the two agree on every output; the geometry's limits are checked beside them.
//   interp_index [n_max m_max]     prints {"pairs": .., "outputs": .., "float_bound_pairs": .., "failures": ..}
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../dspeed_amd/csrc/dsp_kernels.h"
#include "../dspeed_amd/csrc/dsp_program.h"

namespace {

using namespace dsp_interp;

struct Cell {
    int seg;
    Kind kind;
};

// the reference's loops: which segment wrote output o last (NONE: nothing did, the NaN of w_out[:] = nan stays)
std::vector<Cell> forward(int mode, int n, int m) {
    std::vector<Cell> out((size_t)m, Cell{-1, NONE});
    const double upsample = (double)m / (double)n;
    auto fill = [&](long lo, long hi, int seg, Kind kind) {  // w_out[lo:hi] = ..., a slice: clipped to the row
        for (long o = lo < 0 ? 0 : lo; o < hi && o < m; ++o) out[(size_t)o] = Cell{seg, kind};
    };
    if (mode == 'i') {
        for (int i_in = 0; i_in < n; ++i_in) {
            const long i_out = (long)(upsample * i_in);
            out[(size_t)i_out] = Cell{i_in, VALUE};
            fill(i_out + 1, (long)((double)i_out + upsample), i_in, ZERO);  // (the float bound, truncated)
        }
    } else if (mode == 'n' || mode == 'c') {
        long i_last = 0;
        for (int i_in = 0; i_in < n; ++i_in) {
            const long i_next = mode == 'n' ? (long)std::ceil(upsample * (i_in + 0.5)) : (long)std::floor(upsample * i_in) + 1;
            fill(i_last, i_next, i_in, VALUE);
            i_last = i_next;
        }
        fill(i_last, m, n - 1, TAIL);
    } else if (mode == 'f' || mode == 'l') {
        long i_last = 0;
        for (int i_in = 0; i_in < n; ++i_in) {
            const long i_next = (long)std::ceil(upsample * (i_in + 1));
            fill(i_last, i_next, i_in, VALUE);
            i_last = i_next;
        }
    } else if (mode == 'h') {
        long i_last = 0;
        int i_in = 0;
        for (i_in = 0; i_in < n - 1; ++i_in) {
            const long i_next = (long)std::ceil(upsample * (i_in + 1));
            fill(i_last, i_next, i_in, VALUE);
            i_last = i_next;
        }
        fill(i_last, m, n - 2, VALUE);  // (i_in keeps its last value, n - 2: the last segment, extrapolated)
    } else {
        long i_last = m;
        for (int i_in = n - 2; i_in >= 0; --i_in) {
            const long i_next = (long)std::ceil(upsample * i_in);
            for (long o = i_last; o >= i_next; --o)
                if (o < m) out[(size_t)o] = Cell{i_in, VALUE};  // (o == m: the store past the end, dropped)
            i_last = i_next;
        }
    }
    return out;
}

long failures = 0;
void fail(const char* what, int mode, int n, int m, long o, int a, int b) {
    if (++failures <= 20) std::printf("%s: mode %c n %d m %d output %ld: %d, the reference %d\n", what, mode, n, m, o, a, b);
}

}  // namespace

int main(int argc, char** argv) {
    const int n_max = argc > 1 ? std::atoi(argv[1]) : 130, m_max = argc > 2 ? std::atoi(argv[2]) : 400;
    long pairs = 0, outputs = 0, float_pairs = 0;
    const char modes[] = "infclhs";
    for (int n = 1; n <= n_max; ++n)
        for (int m = 1; m <= m_max; ++m) {
            ++pairs;
            bool differs = false;  // from the rational bound ceil(m i / n), at some i < n
            for (int i = 1; i < n && !differs; ++i) differs = ceil_of(ratio(n, m) * (double)i) != ((int64_t)m * i + n - 1) / n;
            float_pairs += differs;
            for (const char* mp = modes; *mp; ++mp) {
                const int mode = *mp;
                if ((mode == 'i' && m % n) || (mode == 'h' && n < 2)) continue;
                const std::vector<Cell> ref = forward(mode, n, m);
                const double u = ratio(n, m);
                int walk = 0;
                for (long o = 0; o < m; ++o) {
                    ++outputs;
                    const Map got = map(mode, n, m, o);
                    const Cell& want = ref[(size_t)o];
                    if (got.kind != want.kind) fail("kind", mode, n, m, o, got.kind, want.kind);
                    if (want.kind != NONE && got.seg != want.seg) fail("segment", mode, n, m, o, got.seg, want.seg);
                    if (got.kind != NONE && (got.seg < 0 || got.seg >= n || ((mode == 'h' || mode == 's') && got.seg > n - 2)))
                        fail("a segment outside the row", mode, n, m, o, got.seg, n);
                    if (mode != 'i') {  // the kernel's walk along consecutive outputs: locate once (every 4th here), advance after it
                        walk = o % 4 == 0 ? locate(mode, n, u, o) : advance(mode, n, u, o, walk);
                        const Map w = map_of(mode, n, m, o, walk);
                        if (w.seg != got.seg || w.kind != got.kind) fail("walk", mode, n, m, o, w.seg, got.seg);
                    }
                }
            }
        }
    // the geometry: the limits the planner names are what the LDS holds, and the switch between the geometries is where a row's bytes say
    static_assert(max_len('l', 4) == DSP_INTERP_F32_MAX && max_len('c', 8) == DSP_INTERP_F32_MAX / 2, "limits");
    static_assert(max_len('s', 4) == DSP_INTERP_SPLINE_F32_MAX && max_len('s', 8) == DSP_INTERP_SPLINE_F64_MAX, "spline limits");
    for (const char* mp = modes; *mp; ++mp)
        for (int esz = 4; esz <= 8; esz += 4)
            for (int n = 1; n <= max_len(*mp, esz); ++n) {
                const int lds = lds_bytes(*mp, n, esz);
                if (lds > LDS_MAX + 16 || (wide(*mp, n, esz) ? lds != row_bytes(*mp, n, esz) + 16 : lds > 4 * WAVE_ROW_BYTES) || w2_offset(n, esz) % 16 ||
                    w2_offset(n, esz) < n * esz || row_bytes(*mp, n, esz) < w2_offset(n, esz) + (*mp == 's' ? n * 8 : 0))
                    fail("geometry", *mp, n, esz, 0, lds, LDS_MAX);
            }
    std::printf("{\"pairs\": %ld, \"outputs\": %ld, \"float_bound_pairs\": %ld, \"failures\": %ld}\n", pairs, outputs, float_pairs, failures);
    return failures ? 1 : 0;
}
