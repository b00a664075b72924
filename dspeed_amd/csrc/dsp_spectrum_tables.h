// dsp_spectrum_tables.h -- the tables of dsp_spectrum.hip, computed on the host in float64 (dsp_chain_create rounds them once to the loop's
// type and uploads them; no launch touches them again).  (re, im) pairs.  No HIP: plain C++17.  Internal header.
//
//   twiddle   exp(-2 pi i k / L), k < L / 2, for the transform of L complex points
//   unpack    exp(-2 pi i k / n), k <= n / 2: a power-of-two row of n samples runs as n / 2 packed points, this step takes them apart
//   chirp     exp(-i pi j^2 / n), j < n: Bluestein's chirp, j^2 reduced modulo 2 n in integers before an angle is formed
//   filter    the spectrum of the conjugate chirp, wrapped into L points, divided by L (the inverse transform's factor: a power of two) and
//             stored in bit-reversed order -- where the forward transform (natural order in, bit-reversed out) leaves its bins
//
// Every angle is a whole number of N-ths of a turn; the multiples of a quarter turn give exactly 1, -i, -1, i.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace dsp_spectrum_tables {

// exp(-2 pi i k / N) into (re, im)
inline void unit(int64_t k, int64_t N, double& re, double& im) {
    k %= N;
    if (k < 0) k += N;
    if (4 * k % N == 0) {  // a whole number of quarter turns
        const double qr[4] = {1.0, 0.0, -1.0, 0.0}, qi[4] = {0.0, -1.0, 0.0, 1.0};
        re = qr[4 * k / N];
        im = qi[4 * k / N];
        return;
    }
    const double a = -2.0 * M_PI * (double)k / (double)N;
    re = cos(a);
    im = sin(a);
}

inline std::vector<double> twiddle(int L) {
    std::vector<double> t((size_t)(L / 2) * 2);
    for (int k = 0; k < L / 2; ++k) unit(k, L, t[2 * k], t[2 * k + 1]);
    return t;
}

inline std::vector<double> unpack(int n) {
    std::vector<double> t((size_t)(n / 2 + 1) * 2);
    for (int k = 0; k <= n / 2; ++k) unit(k, n, t[2 * k], t[2 * k + 1]);
    return t;
}

inline std::vector<double> chirp(int n) {
    std::vector<double> t((size_t)n * 2);
    for (int64_t j = 0; j < n; ++j) unit(j * j % (2 * (int64_t)n), 2 * (int64_t)n, t[2 * j], t[2 * j + 1]);
    return t;
}

inline unsigned bit_reverse(unsigned v, int bits) {
    unsigned r = 0;
    for (int b = 0; b < bits; ++b) r |= ((v >> b) & 1u) << (bits - 1 - b);
    return r;
}

// in place, natural order in and out: bit reversal, then the passes of growing span
inline void fft_f64(std::vector<double>& z, int L, int bits) {
    for (unsigned i = 0; i < (unsigned)L; ++i) {
        const unsigned j = bit_reverse(i, bits);
        if (i < j) {
            std::swap(z[2 * i], z[2 * j]);
            std::swap(z[2 * i + 1], z[2 * j + 1]);
        }
    }
    for (int h = 1; h < L; h *= 2)
        for (int b = 0; b < L; b += 2 * h)
            for (int k = 0; k < h; ++k) {
                double wr, wi;
                unit(k, 2 * (int64_t)h, wr, wi);
                const int i = b + k, j = i + h;
                const double tr = z[2 * j] * wr - z[2 * j + 1] * wi, ti = z[2 * j] * wi + z[2 * j + 1] * wr;
                z[2 * j] = z[2 * i] - tr;
                z[2 * j + 1] = z[2 * i + 1] - ti;
                z[2 * i] += tr;
                z[2 * i + 1] += ti;
            }
}

inline std::vector<double> filter(int n, int L, int bits) {
    std::vector<double> b((size_t)L * 2, 0.0);
    const std::vector<double> c = chirp(n);
    for (int j = 0; j < n; ++j) {  // conj(chirp[|j|]) at j and at -j, wrapped
        b[2 * j] = c[2 * j];
        b[2 * j + 1] = -c[2 * j + 1];
        if (j) {
            b[2 * (L - j)] = c[2 * j];
            b[2 * (L - j) + 1] = -c[2 * j + 1];
        }
    }
    fft_f64(b, L, bits);
    std::vector<double> out((size_t)L * 2);
    for (unsigned p = 0; p < (unsigned)L; ++p) {
        const unsigned k = bit_reverse(p, bits);
        out[2 * p] = b[2 * k] / L;
        out[2 * p + 1] = b[2 * k + 1] / L;
    }
    return out;
}

}  // namespace dsp_spectrum_tables
