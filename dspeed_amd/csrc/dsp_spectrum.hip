// dsp_spectrum.hip -- psd and fft (processors/fft.py:92-126, 12-46): the real spectrum of a row, X[k] = sum_j w[j] exp(-2 pi i j k / n) for
// k = 0 .. n / 2 (NumPy's rfft: no normalisation), as it stands (fft: (re, im) pairs) or as (re^2 + im^2) / n (psd).
//
// One row is one transform of L complex points (L a power of two), held in LDS as (re, im) pairs of the loop's type for all of its passes.
//   geometry   rows whose transform fills up to 8 KiB get a wavefront each, four to a workgroup, and need no barrier; longer ones a
//              workgroup of 256 (dsp_kernels.h, dsp_spectrum).  Both are this one kernel: WIDE chooses what "everybody" means.  A wide
//              row's four wavefronts agree on "a NaN or an infinity" through one word behind the transform (16 bytes past the 64 KiB of
//              the longest rows: dsp_internal_set_spectrum_lds).
//   staging    the shared loader (dsp_row_stream.h): 16 bytes per lane and load where start, stride and length allow, else a sample per lane.
//              The pass also finds "a NaN or an infinity" of the row: such a row's bins are all NaN (fft: real part NaN, imaginary part 0).
//   n = 2^p    the row is packed as n / 2 points z[j] = w[2 j] + i w[2 j + 1], transformed (natural order in, bit-reversed order out), and
//              taken apart behind it: with E = (Z[k] + conj Z[L - k]) / 2 and O = -i (Z[k] - conj Z[L - k]) / 2, X[k] = E + exp(-2 pi i k / n) O;
//              X[0] = E + O and X[n / 2] = E - O of Z[0] need no table.  n = 2 and 4 are the same code with L = 1 and 2; n = 1 is X[0] = w[0].
//   other n    Bluestein: a[j] = w[j] chirp[j], zeros up to L >= 2 n - 1; the transform; times the spectrum of the conjugate chirp, which the
//              table holds in the bit-reversed order the transform leaves (with the inverse's 1 / L in it); the inverse transform, whose
//              passes take bit-reversed order back to natural with conjugate twiddles; X[k] = chirp[k] y[k].  No pass reorders anything.
//   passes     radix 2, in place: pass of span h pairs point i (bit h clear) with i + h, a butterfly per thread and step.
//   banks      point i lives at swz(i): its low five bits -- the 8-byte bank pair of a float32 point -- are i's XOR 31 where bit 5 is set,
//              XOR bits 6 .. 10, XOR bits 11 .. 15.  The 32 points a half wavefront reads together then lie in 32 different bank pairs in
//              each of the three patterns there are: 32 neighbours (long spans, staging, the filter); five of the low six bits varying,
//              the sixth the pass's own (spans below 32, two-way conflicts in the plain order); and the bit-reversed neighbours of the
//              unpacking step, whose top five bits vary (one bank pair for all 32 in the plain order): any five consecutive bits above
//              bit 5 map onto the five bank bits one to one, and bit 5's 31 keeps the middle pattern apart from them.
//   tables     twiddles, unpacking twiddles, chirp and filter are the chain's (dsp_spectrum_tables.h): read here, never written.
#include <hip/hip_runtime.h>

#include "dsp_kernels.h"
#include "dsp_launch.h"
#include "dsp_row_stream.h"
#include "dsp_wave.h"

namespace {

template <typename T>
struct Cx {
    T re, im;
};
template <typename T>
__device__ __forceinline__ Cx<T> mul(Cx<T> a, Cx<T> b) {
    return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
template <typename T>
__device__ __forceinline__ Cx<T> mul_conj(Cx<T> a, Cx<T> b) {  // a conj(b)
    return {a.re * b.re + a.im * b.im, a.im * b.re - a.re * b.im};
}

__device__ __forceinline__ int swz(int i) { return i ^ ((i & 32) ? 31 : 0) ^ ((i >> 6) & 31) ^ ((i >> 11) & 31); }

// N: samples per lane and load (dsp_row_stream.h); WIDE: a workgroup per row, else a wavefront
template <typename T, typename IN, int N, bool WIDE>
__global__ void __launch_bounds__(256) dsp_spectrum_kernel(SpectrumArgs A, int64_t n_wf) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int K = N > 1 ? 4 : 8;        // loads in flight
    constexpr int G = WIDE ? 256 : 64;      // threads of a row
    constexpr int NW = WIDE ? 4 : 1;        // wavefronts of a row
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const int tid = WIDE ? (int)threadIdx.x : lane;
    const int64_t row = WIDE ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + wave;
    if (!WIDE && row >= n_wf) return;  // (whole wavefronts, and no barrier in this geometry; WIDE: the grid is n_wf)
    const int n = A.len, m = A.m, L = A.points;
    Cx<T>* z = (Cx<T>*)lds_raw + (WIDE ? 0 : wave * L);
    int* row_bad = (int*)((Cx<T>*)lds_raw + L);  // (WIDE)
    const IN* w = (const IN*)A.wf + row * A.wf_stride + A.wf_offset;
    const Cx<T>* tw = (const Cx<T>*)A.twiddle;
    const Cx<T>* aux = (const Cx<T>*)A.aux;
    auto everybody = [&]() {
        if constexpr (WIDE)
            __syncthreads();
        else
            wave_sync();
    };

    // staging
    if constexpr (WIDE) {
        if (tid == 0) *row_bad = 0;
        __syncthreads();
    }
    if (A.bluestein)
        for (int i = n + tid; i < L; i += G) z[swz(i)] = {(T)0, (T)0};
    bool bad = false;
    for (int g0 = (WIDE ? wave : 0) * K; g0 < row_groups<N>(n); g0 += NW * K) {
        T x[K][N];
        load_row_groups<T, IN, N, K>(x, w, n, g0, lane);
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const int s = in_row<N>(g0, k, j, lane);
                if (s >= n) continue;
                const T v = x[k][j];
                bad |= !(v - v == (T)0);  // a NaN or an infinity
                if (A.bluestein) {
                    const Cx<T> c = aux[s];
                    z[swz(s)] = {v * c.re, v * c.im};
                } else if (n == 1) {
                    z[0] = {v, (T)0};
                } else if constexpr (N == 1) {
                    ((T*)&z[swz(s >> 1)])[s & 1] = v;
                } else if ((j & 1) == 0) {  // (whole vectors of an even number of samples: a point at a time)
                    z[swz(s >> 1)] = {v, x[k][j + 1 < N ? j + 1 : j]};
                }
            }
    }
    bad = wave_any(bad);
    if constexpr (WIDE) {
        if (bad && lane == 0) *row_bad = 1;
        __syncthreads();  // (also the barrier behind the staging)
        bad = *row_bad != 0;
    } else {
        wave_sync();
    }

    T* out = (T*)A.out + row * A.out_stride;
    if (bad) {
        const T nanv = quiet_nan<T>();
        for (int k = tid; k < m; k += G) {
            if (A.complex_out) {
                out[2 * k] = nanv;
                out[2 * k + 1] = (T)0;
            } else {
                out[k] = nanv;
            }
        }
        return;  // (everybody of the row: `bad` is the row's)
    }

    // forward: natural order in, bit-reversed out
    for (int h = L >> 1, step = 1; h >= 1; h >>= 1, step <<= 1) {
        for (int t = tid; t < (L >> 1); t += G) {
            const int k = t & (h - 1), i = ((t - k) << 1) | k;
            const Cx<T> a = z[swz(i)], b = z[swz(i + h)], wk = tw[k * step];
            z[swz(i)] = {a.re + b.re, a.im + b.im};
            z[swz(i + h)] = mul<T>({a.re - b.re, a.im - b.im}, wk);
        }
        everybody();
    }

    if (A.bluestein) {
        const Cx<T>* filter = (const Cx<T>*)A.filter;
        for (int p = tid; p < L; p += G) z[swz(p)] = mul(z[swz(p)], filter[p]);
        everybody();
        // inverse: bit-reversed order in, natural out, conjugate twiddles (its 1 / L is the filter's)
        for (int h = 1, step = L >> 1; h < L; h <<= 1, step >>= 1) {
            for (int t = tid; t < (L >> 1); t += G) {
                const int k = t & (h - 1), i = ((t - k) << 1) | k;
                const Cx<T> a = z[swz(i)], b = mul_conj(z[swz(i + h)], tw[k * step]);
                z[swz(i)] = {a.re + b.re, a.im + b.im};
                z[swz(i + h)] = {a.re - b.re, a.im - b.im};
            }
            everybody();
        }
    }

    // the bins: coalesced scalar stores (rows of n / 2 + 1 values keep no alignment)
    const T len_t = (T)n;
    for (int k = tid; k < m; k += G) {
        Cx<T> X;
        if (A.bluestein) {
            X = mul(z[swz(k)], aux[k]);
        } else if (n == 1) {
            X = z[0];
        } else {
            const int bits = A.log2_points;
            auto at = [&](int q) { return z[swz(bits ? (int)(__brev((unsigned)q) >> (32 - bits)) : 0)]; };
            const Cx<T> p = at(k & (L - 1)), q = at((L - k) & (L - 1));
            const Cx<T> E = {(T)0.5 * (p.re + q.re), (T)0.5 * (p.im - q.im)}, O = {(T)0.5 * (p.im + q.im), (T)0.5 * (q.re - p.re)};
            if (k == 0)
                X = {E.re + O.re, (T)0};
            else if (k == L)
                X = {E.re - O.re, (T)0};
            else {
                const Cx<T> u = mul(O, aux[k]);
                X = {E.re + u.re, E.im + u.im};
            }
        }
        if (A.complex_out) {
            out[2 * k] = X.re;
            out[2 * k + 1] = X.im;
        } else {
            out[k] = (X.re * X.re + X.im * X.im) / len_t;
        }
    }
}

template <typename T, typename IN>
void launch_spectrum(const SpectrumArgs* A, int64_t n_wf, int vec, int lds_bytes, hipStream_t stream) {
#define DSP_SPECTRUM_LAUNCH(NV, WIDE, BLOCKS) \
    hipLaunchKernelGGL((dsp_spectrum_kernel<T, IN, NV, WIDE>), dim3(BLOCKS), dim3(256), lds_bytes, stream, *A, n_wf)
    if (A->wide) {
        if (vec)
            DSP_SPECTRUM_LAUNCH(RowVec<IN>::N, true, (unsigned)n_wf);
        else
            DSP_SPECTRUM_LAUNCH(1, true, (unsigned)n_wf);
    } else {
        if (vec)
            DSP_SPECTRUM_LAUNCH(RowVec<IN>::N, false, row_blocks(n_wf));
        else
            DSP_SPECTRUM_LAUNCH(1, false, row_blocks(n_wf));
    }
#undef DSP_SPECTRUM_LAUNCH
}

}  // namespace

template <typename T, typename IN>
int set_lds(int lds_bytes) {
    int rc = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(&dsp_spectrum_kernel<T, IN, RowVec<IN>::N, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (rc) return rc;
    return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(&dsp_spectrum_kernel<T, IN, 1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
}

extern "C" int dsp_internal_set_spectrum_lds(int dtype, int lds_bytes) {
    switch (dtype) {
        case DSP_F32: return set_lds<float, float>(lds_bytes);
        case DSP_I16: return set_lds<float, int16_t>(lds_bytes);
        case DSP_U16: return set_lds<float, uint16_t>(lds_bytes);
        default: return set_lds<double, double>(lds_bytes);
    }
}

extern "C" int dsp_internal_launch_spectrum(const SpectrumArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream) {
    (void)err;  // (no row of this kernel is a DSPFatal)
    if (n_wf <= 0) return 0;
    const int esz = dtype == DSP_F64 ? 8 : 4;
    // (the planner's bounds, once more where the LDS is sized: the transform the plan names is the row's, and a workgroup's 64 KiB hold it)
    if (A->len < 1 || A->m != A->len / 2 + 1 || A->points != dsp_spectrum::points(A->len) || (1 << A->log2_points) != A->points ||
        A->bluestein != (dsp_spectrum::pow2(A->len) ? 0 : 1) || A->wide != (dsp_spectrum::wide(A->len, esz) ? 1 : 0) ||
        dsp_spectrum::row_bytes(A->len, esz) > 64 * 1024 || n_wf > 0x7fffffff || !A->aux || (A->points > 1 && !A->twiddle) || (A->bluestein && !A->filter))
        return (int)hipErrorInvalidValue;
    const int lds = dsp_spectrum::lds_bytes(A->len, esz);
    switch (dtype) {
        case DSP_F32: launch_spectrum<float, float>(A, n_wf, vec, lds, stream); break;
        case DSP_I16: launch_spectrum<float, int16_t>(A, n_wf, vec, lds, stream); break;
        case DSP_U16: launch_spectrum<float, uint16_t>(A, n_wf, vec, lds, stream); break;
        case DSP_F64: launch_spectrum<double, double>(A, n_wf, vec, lds, stream); break;
        default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}
