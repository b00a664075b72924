// dsp_dense.hip -- the neural-network layers of processors/ml.py: normalisation_layer, dense_layer_no_bias / _with_bias and
// classification_layer_no_bias / _with_bias.  A dense layer over a batch is rows x an (n, m) weight matrix: the one GEMM-shaped processor,
// on the matrix cores in full precision (v_mfma_f32_16x16x4_f32 in the float32 loop, v_mfma_f64_16x16x4_f64 in the float64 loop).
//   geometry   a workgroup of 4 wavefronts takes 64 rows and all m outputs; a wavefront 16 rows x m, m in blocks of 16 columns, one accumulator
//              tile per block in registers (NB of them: the kernel is built for 1, 4 and 16 blocks).  Geometry and LDS layout are
//              dsp_kernels.h's, dsp_dense, shared with the planner.
//   staging    rows pass through LDS in chunks of 256 bytes along n, through the shared loader (dsp_row_stream.h): every wavefront stages its own
//              16 rows, 16 bytes a lane where stride, offset and length allow, a sample a lane elsewhere.  The weights' chunk is staged beside
//              them by the whole workgroup; they are re-read per workgroup and expected to stay in L2.  Whatever lies beyond n (in k), beyond
//              m (in the weights' columns) and beyond the batch (in the rows) is ZERO in LDS, in both operands: 0 x garbage may be NaN.
//   order      one accumulator per output; k ascends from 0 in steps of the instruction's depth (4) and inside the instruction, no split-k: the
//              float32 result is one fmaf chain in ascending k from +0 (a zero product behind the end of the row leaves the sum as it is).
//              The bias is added behind the chain as one addition of the loop's type.
//   NaN rule   the reference writes NaNs for a row that holds a NaN.  No scan is needed for that: every output of the row sums a product with
//              the NaN sample, and NaN x w is NaN for every w, 0 and infinities included, so every output comes out NaN through the products.
//   activation numba's typing of the reference's own gufuncs (relu, leaky_relu, sigmoid, softmax = softplus) and NumPy's of tanh, the
//              expressions as written: in the float32 loop exp is float32, `0.01 * x`, `1 + exp` and `1 / (...)` are float64, the store rounds
//              once.  A character that is none of "srlmt" leaves NaNs, as the reference does.
//   normalise  (x - means[k]) / sqrt(variances[k]) in the loop's type, IEEE division and square root, applied while a row is staged (the fused
//              form) or by dsp_normalise_kernel, a wavefront per row, when the normalised row itself is the result: one expression, the same bits.
#include <hip/hip_runtime.h>

#include "dsp_kernels.h"
#include "dsp_launch.h"
#include "dsp_row_stream.h"
#include "dsp_wave.h"

namespace {

using namespace dsp_dense;

template <typename T>
struct Mma;
template <>
struct Mma<float> {
    typedef float acc __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc fma(float a, float b, acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) * 4 + reg; }  // (column: lane & 15)
};
template <>
struct Mma<double> {
    typedef double acc __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc fma(double a, double b, acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) + 4 * reg; }  // (the float64 form has a map of its own)
};

template <typename T>
__device__ __forceinline__ T normalised(T x, T mean, T variance) {
    return (x - mean) / sqrt(variance);
}

__device__ __forceinline__ float activate(float v, int act) {
    switch (act) {
        case 'r': return v * (v > 0.0f ? 1.0f : 0.0f);  // (-0.0 below zero, NaN at -inf: the expression as written)
        case 'l': return (float)((double)(v * (v > 0.0f ? 1.0f : 0.0f)) + (0.01 * (double)v) * (v < 0.0f ? 1.0 : 0.0));
        case 's': return (float)(1.0 / (1.0 + (double)expf(-v)));
        case 'm': return (float)log(1.0 + (double)expf(v));
        case 't': return tanhf(v);
        default: return quiet_nan<float>();
    }
}
__device__ __forceinline__ double activate(double v, int act) {
    switch (act) {
        case 'r': return v * (v > 0.0 ? 1.0 : 0.0);
        case 'l': return v * (v > 0.0 ? 1.0 : 0.0) + (0.01 * v) * (v < 0.0 ? 1.0 : 0.0);
        case 's': return 1.0 / (1.0 + exp(-v));
        case 'm': return log(1.0 + exp(v));
        case 't': return tanh(v);
        default: return quiet_nan<double>();
    }
}

// The weights' chunk -- rows k0 .. k0 + chunk of (n, m) -- into wl[chunk][WP], zero beyond n and m.  VW values a load and LDS write: 16 bytes
// where m is a multiple of them and the matrix starts on a 16-byte boundary (a vector then lies inside m whole or beyond it whole), one
// otherwise.  A thread requests up to 8 loads before it writes the first; its (k, column) advances by 256 vectors a turn without a
// division.
template <typename T, int VW, int NB>
__device__ __forceinline__ void stage_weights(T* wl, const T* W, int k0, int kc, int m, int cols, int WP, int tid) {
    constexpr int KC = chunk((int)sizeof(T)), TURNS = KC * NB * BLOCK / VW / 256;
    typedef T Vec __attribute__((ext_vector_type(VW > 1 ? VW : 2)));
    const int cv = cols / VW;  // vectors of an LDS row
    int k = tid / cv, j = tid - k * cv;
    const int dk = 256 / cv, dj = 256 - dk * cv;
    constexpr int BATCH = TURNS < 8 ? TURNS : 8;
    static_assert(TURNS % BATCH == 0, "whole batches");
#pragma unroll 1
    for (int t0 = 0; t0 < TURNS; t0 += BATCH) {
    T v[BATCH][VW];
    int at[BATCH];
#pragma unroll
    for (int t = 0; t < BATCH; ++t) {
        at[t] = k < KC ? k * WP + j * VW : -1;
#pragma unroll
        for (int i = 0; i < VW; ++i) v[t][i] = (T)0;
        if (k < kc && j * VW < m) {
            const T* from = W + (int64_t)(k0 + k) * m + j * VW;
            if constexpr (VW > 1) {
                const Vec q = *(const Vec*)from;
#pragma unroll
                for (int i = 0; i < VW; ++i) v[t][i] = q[i];
            } else {
                v[t][0] = *from;
            }
        }
        k += dk, j += dj;
        if (j >= cv) j -= cv, ++k;
    }
#pragma unroll
    for (int t = 0; t < BATCH; ++t) {
        if (at[t] < 0) continue;
        if constexpr (VW > 1) {
            Vec q;
#pragma unroll
            for (int i = 0; i < VW; ++i) q[i] = v[t][i];
            *(Vec*)(wl + at[t]) = q;
        } else {
            wl[at[t]] = v[t][0];
        }
    }
    }
}

// N: samples per lane and load (dsp_row_stream.h); NB: accumulator tiles (column blocks) a wavefront is built for
template <typename T, typename IN, int N, int NB>
__global__ void __launch_bounds__(256) dsp_dense_kernel(DenseArgs A, int64_t n_wf) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int KC = chunk((int)sizeof(T)), XP = x_pitch((int)sizeof(T));
    // rows requested before the first is looked at.  The widest build runs a workgroup a CU (87 KiB of LDS): all of a wavefront's rows at once
    // hide the memory's latency there (2.03 -> 1.87 ms per 131 072 rows at 1024 -> 256); the narrow builds have the workgroups for that, and
    // more registers cost them residency (0.31 -> 0.47 ms at 1024 -> 1)
    constexpr int RQ = NB == BLOCKS_MAX && N <= 4 ? WAVE_ROWS : 4;
    typedef typename Mma<T>::acc Acc;
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6), tid = (int)threadIdx.x;
    const int n = A.len, m = A.m, nbu = blocks(m), WP = w_pitch(m), cols = nbu * BLOCK;
    T* wl = (T*)lds_raw;                            // [KC][WP]
    T* xw = wl + KC * WP + wave * WAVE_ROWS * XP;   // [WAVE_ROWS][XP]: this wavefront's rows
    const int64_t row0 = (int64_t)blockIdx.x * TILE_ROWS + wave * WAVE_ROWS;
    const IN* w = (const IN*)A.wf + A.wf_offset;
    const T* W = (const T*)A.weights;
    const bool w_vec = m % (16 / (int)sizeof(T)) == 0 && ((uintptr_t)W & 15u) == 0;
    const T *means = (const T*)A.means, *variances = (const T*)A.variances;

    Acc acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = Acc{0, 0, 0, 0};

    for (int k0 = 0; k0 < n; k0 += KC) {
        const int kc = n - k0 < KC ? n - k0 : KC;
        if (w_vec)
            stage_weights<T, 16 / (int)sizeof(T), NB>(wl, W, k0, kc, m, cols, WP, tid);
        else
            stage_weights<T, 1, NB>(wl, W, k0, kc, m, cols, WP, tid);
        // this wavefront's rows: the loader leaves 0 in the lanes beyond kc, and in every lane of a row beyond the batch (which is not read)
#pragma unroll
        for (int r0 = 0; r0 < WAVE_ROWS; r0 += RQ) {
            T s[RQ][1][N];
#pragma unroll
            for (int q = 0; q < RQ; ++q) {
                const int64_t row = row0 + r0 + q;
                load_row_groups<T, IN, N, 1>(s[q], w + row * A.wf_stride + k0, row < n_wf ? kc : 0, 0, lane);
            }
            const int at = lane * N;
            if (at < KC) {
#pragma unroll
                for (int q = 0; q < RQ; ++q)
#pragma unroll
                    for (int j = 0; j < N; ++j) {
                        T v = s[q][0][j];
                        if (A.normalise && at + j < kc && row0 + r0 + q < n_wf) v = normalised(v, means[k0 + at + j], variances[k0 + at + j]);
                        xw[(r0 + q) * XP + at + j] = v;
                    }
            }
        }
        __syncthreads();
        const int steps = (kc + DEPTH - 1) / DEPTH;
        for (int kk = 0; kk < steps; ++kk) {
            const int k = kk * DEPTH + (lane >> 4);
            const T a = xw[(lane & 15) * XP + k];
#pragma unroll
            for (int b = 0; b < NB; ++b)
                if (b < nbu) acc[b] = Mma<T>::fma(a, wl[k * WP + b * BLOCK + (lane & 15)], acc[b]);
        }
        __syncthreads();
    }

    const T* bias = (const T*)A.bias;
    T* out = (T*)A.out;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int j = b * BLOCK + (lane & 15);
        if (b >= nbu || j >= m) continue;
        const T bj = bias ? bias[j] : (T)0;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t row = row0 + Mma<T>::row(lane, reg);
            if (row >= n_wf) continue;
            T v = acc[b][reg];
            if (bias) v = v + bj;
            out[row * A.out_stride + j] = activate(v, A.activation);
        }
    }
}

// the normalised row itself as the result: a wavefront per row, four rows to a workgroup
template <typename T, typename IN, int N>
__global__ void __launch_bounds__(256) dsp_normalise_kernel(DenseArgs A, int64_t n_wf) {
    constexpr int K = N > 1 ? 4 : 8;  // loads in flight
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= n_wf) return;
    const int n = A.len;
    const IN* w = (const IN*)A.wf + row * A.wf_stride + A.wf_offset;
    const T *means = (const T*)A.means, *variances = (const T*)A.variances;
    T* out = (T*)A.out + row * A.out_stride;
    for (int g0 = 0; g0 < row_groups<N>(n); g0 += K) {
        T s[K][N];
        load_row_groups<T, IN, N, K>(s, w, n, g0, lane);
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const int at = in_row<N>(g0, k, j, lane);
                if (at < n) out[at] = normalised(s[k][j], means[at], variances[at]);
            }
    }
}

template <typename T, typename IN, int N>
void launch_dense_n(const DenseArgs* A, int64_t n_wf, int lds_bytes, hipStream_t stream) {
    if (A->m < 1) {
        hipLaunchKernelGGL((dsp_normalise_kernel<T, IN, N>), dim3(row_blocks(n_wf)), dim3(256), 0, stream, *A, n_wf);
        return;
    }
    const dim3 grid((unsigned)tiles(n_wf));
    switch (built_blocks(A->m)) {
        case 1: hipLaunchKernelGGL((dsp_dense_kernel<T, IN, N, 1>), grid, dim3(256), lds_bytes, stream, *A, n_wf); break;
        case 4: hipLaunchKernelGGL((dsp_dense_kernel<T, IN, N, 4>), grid, dim3(256), lds_bytes, stream, *A, n_wf); break;
        default: hipLaunchKernelGGL((dsp_dense_kernel<T, IN, N, BLOCKS_MAX>), grid, dim3(256), lds_bytes, stream, *A, n_wf); break;
    }
}

template <typename T, typename IN>
void launch_dense(const DenseArgs* A, int64_t n_wf, int vec, int lds_bytes, hipStream_t stream) {
    if (vec)
        launch_dense_n<T, IN, RowVec<IN>::N>(A, n_wf, lds_bytes, stream);
    else
        launch_dense_n<T, IN, 1>(A, n_wf, lds_bytes, stream);
}

// (only the build for BLOCKS_MAX column blocks holds layers whose LDS passes 64 KiB)
template <typename T, typename IN>
int set_lds(int lds_bytes) {
    const void* kernels[] = {reinterpret_cast<const void*>(&dsp_dense_kernel<T, IN, RowVec<IN>::N, BLOCKS_MAX>),
                             reinterpret_cast<const void*>(&dsp_dense_kernel<T, IN, 1, BLOCKS_MAX>)};
    for (const void* k : kernels)
        if (int rc = (int)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes)) return rc;
    return 0;
}

}  // namespace

extern "C" int dsp_internal_set_dense_lds(int dtype, int lds_bytes) {
    switch (dtype) {
        case DSP_F32: return set_lds<float, float>(lds_bytes);
        case DSP_I16: return set_lds<float, int16_t>(lds_bytes);
        case DSP_U16: return set_lds<float, uint16_t>(lds_bytes);
        default: return set_lds<double, double>(lds_bytes);
    }
}

extern "C" int dsp_internal_launch_dense(const DenseArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream) {
    (void)err;  // (no row of these kernels is a DSPFatal)
    if (n_wf <= 0) return 0;
    const int esz = dtype == DSP_F64 ? 8 : 4;
    // (the planner's bounds, once more where the LDS is sized and the accumulators are counted)
    if (A->len < 1 || A->len > N_MAX || A->m < 0 || A->m > M_MAX || (A->m > 0 && !A->weights) || (A->m == 0 && !A->normalise) ||
        (A->normalise && (!A->means || !A->variances)) || tiles(n_wf) > 0x7fffffff || (A->m == 0 && n_wf > 4 * (int64_t)0x7fffffff))
        return (int)hipErrorInvalidValue;
    const int lds = lds_bytes(A->m, esz);
    switch (dtype) {
        case DSP_F32: launch_dense<float, float>(A, n_wf, vec, lds, stream); break;
        case DSP_I16: launch_dense<float, int16_t>(A, n_wf, vec, lds, stream); break;
        case DSP_U16: launch_dense<float, uint16_t>(A, n_wf, vec, lds, stream); break;
        case DSP_F64: launch_dense<double, double>(A, n_wf, vec, lds, stream); break;
        default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}
