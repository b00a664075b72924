// ml_fma.cpp -- the accumulation rule of dsp_dense.hip on the host, for tests/ml_cases.py: every output of a dense layer is ONE fused
// multiply-add chain in ascending k from +0, fmaf in the float32 loop and fma in the float64 loop (v_mfma_f32_16x16x4_f32 is such a chain
// bit for bit).  Python 3.10 has no math.fma, and a float64 product-and-add rounded twice is not the same function.
//
//   ml_fma <in> <out>
// <in>:  int32 header {is_f64, rows, n, m}, then x (rows x n) and w (n x m), row-major, float32 or float64.
// <out>: the pre-activations (rows x m) of the same type: no bias, no activation.
// Plain C++, no HIP.  Built with -ffp-contract=off: the only fused operations are the ones written.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

template <typename T>
static int run(FILE* in, FILE* out, int rows, int n, int m) {
    std::vector<T> x((size_t)rows * n), w((size_t)n * m), y((size_t)rows * m);
    if (fread(x.data(), sizeof(T), x.size(), in) != x.size() || fread(w.data(), sizeof(T), w.size(), in) != w.size()) return 3;
    for (int r = 0; r < rows; ++r)
        for (int j = 0; j < m; ++j) {
            T acc = 0;
            for (int k = 0; k < n; ++k) acc = std::fma(x[(size_t)r * n + k], w[(size_t)k * m + j], acc);
            y[(size_t)r * m + j] = acc;
        }
    return fwrite(y.data(), sizeof(T), y.size(), out) == y.size() ? 0 : 4;
}

int main(int argc, char** argv) {
    if (argc != 3) return 1;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    int32_t h[4];
    if (!in || !out || fread(h, sizeof h[0], 4, in) != 4 || h[1] < 0 || h[2] < 0 || h[3] < 0 || h[1] > (1 << 20) || h[2] > (1 << 20) || h[3] > (1 << 20)) return 2;
    const int rc = h[0] ? run<double>(in, out, h[1], h[2], h[3]) : run<float>(in, out, h[1], h[2], h[3]);
    fclose(in);
    return fclose(out) == 0 ? rc : 5;
}
