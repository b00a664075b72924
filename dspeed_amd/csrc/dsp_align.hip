// dsp_align.hip -- the waveform aligner, four processors of one family and one launch that joins two of them:
//   inl_correction  (processors/inl_correction.py:12-61): the ADC's integral non-linearity, a table looked up by the sample itself
//   get_wf_centroid (processors/get_wf_centroid.py:12-69): the middle of the zero crossing between a row's minimum and its maximum
//   wf_alignment    (processors/wf_alignment.py:12-87): a window of `size` samples around the centroid
//   wf_correction   (processors/wf_correction.py:10-83): a fixed template subtracted on [start, stop)
//   wf_alignment -> wf_correction in one launch: the window stays in registers, the template is subtracted before the store.
//
// A wavefront per row, four to a workgroup, nothing in LDS (dsp_pulses.hip's geometry).  Nothing here is a chain along the samples: lanes
// share a row's samples, consecutive lanes consecutive addresses.  Every launch reads and writes the least the semantics allow:
//   inl        the row once (dsp_row_stream.h), the table by gather (it lives in L2), the output once.
//   centroid   two passes over memory: the row once for the extremes and the NaN rule, then [lo, hi) only for the first positive and the
//              last negative sample.  The first pass loads without the streaming hint, so that the second may find its samples in the
//              caches; whether it does depends on the row's length and on what else is resident, and is not counted on.  First-occurrence ties hold inside a lane (ascending
//              indices, strict comparison) and across lanes (the index breaks ties in the wave reduction, as min_max has it).
//   window     integer rows cannot hold a NaN: only the `size` samples of the window are read (and w_in[0] in the second branch).  Float
//              rows are read once for the NaN rule (no streaming hint, as for the centroid); the window's samples are then read again.
//   correction the row once, the output once: a row is written as it is read, and written again, as NaNs, only if a NaN turned up.
// A NaN anywhere in a table (inl, w_corr) makes every row NaN: dsp_align_table_kernel looks at the table once per launch, ahead of the
// rows, and leaves a word in device memory (A.table_nan) -- not every wavefront at every entry.
// Where the reference defines no result: dsp_program.h (dsp_align_window) and DESIGN.md -- NaN, no error.  No multiply anywhere.
#include <hip/hip_runtime.h>

#include "dsp_kernels.h"
#include "dsp_launch.h"
#include "dsp_row_stream.h"
#include "dsp_wave.h"

namespace {

template <typename T>
__global__ void __launch_bounds__(256) dsp_align_table_kernel(const T* __restrict__ table, int len, int* flag) {
    bool bad = false;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < len; i += gridDim.x * 256) bad |= table[i] != table[i];
    if (bad) *flag = 1;  // (every writer writes the same word; the launcher cleared it)
}

__device__ __forceinline__ void set_error(int* err, int code, int64_t row) {
    if (atomicCAS(&err[0], 0, code) == 0) {
        err[1] = (int)(row & 0xffffffffll);
        err[2] = (int)(row >> 32);
    }
}

// the N values a lane holds of a group go to out[at .. at + N): one or two 16-byte stores where the launcher vouches for the alignment
template <typename T, int N, bool VEC>
__device__ __forceinline__ void store_lane(T* out, int at, int n, const T (&v)[N]) {
    if constexpr (VEC && N > 1) {
        constexpr int PER = 16 / (int)sizeof(T);
        typedef T vec __attribute__((ext_vector_type(PER)));
        if (at < n) {  // (n is a multiple of N: a lane's values lie inside the row together)
#pragma unroll
            for (int q = 0; q < N / PER; ++q) {
                vec x;
#pragma unroll
                for (int e = 0; e < PER; ++e) x[e] = v[q * PER + e];
                *(vec*)(out + at + q * PER) = x;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (at + j < n) out[at + j] = v[j];
    }
}

// load_row_groups (dsp_row_stream.h) with ordinary loads instead of non-temporal ones: for the passes whose row, or a part of it, is read
// again by the same wavefront (the centroid's [lo, hi), the float rows' window) -- a streaming hint would ask the caches to let go of it
template <typename T, typename IN, int N, int K>
__device__ __forceinline__ void load_row_groups_kept(T (&x)[K][N], const IN* w, int n, int g0, int lane) {
    if constexpr (N > 1) {
        typedef typename RowVec<IN>::vec vec;
        const vec* wv = (const vec*)w;
        vec v[K] = {};
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (in_row<N>(g0, k, 0, lane) < n) v[k] = wv[(g0 + k) * 64 + lane];
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int j = 0; j < N; ++j) x[k][j] = (T)v[k][j];
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int at = in_row<1>(g0, k, 0, lane);
            x[k][0] = at < n ? (T)w[at] : (T)0;
        }
    }
}

template <typename T>
__device__ __forceinline__ void fill_row(T* out, int n, T value, int lane) {
    for (int j = lane; j < n; j += 64) out[j] = value;
}

template <typename IN>
constexpr bool is_float_row = false;
template <>
constexpr bool is_float_row<float> = true;
template <>
constexpr bool is_float_row<double> = true;

// N: samples per lane and load of the streaming passes (1, or those of a 16-byte vector); OV: 16-byte stores of the streamed outputs
template <typename T, typename IN, int N, bool OV>
__global__ void __launch_bounds__(256) dsp_align_kernel(AlignArgs A, int64_t n_wf, int* err) {
    constexpr int K = N > 1 ? 4 : 8;  // loads in flight, streaming passes
    constexpr int U = 8;              // loads in flight, the window and the search between the extremes
    const int lane = lane_id();
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_wf) return;  // (whole wavefronts: no barrier in this kernel)
    const IN* __restrict__ w = (const IN*)A.wf + row * A.wf_stride + A.wf_offset;
    const int n = A.len;
    const T nanv = quiet_nan<T>();
    const bool table_nan = A.table_nan && *A.table_nan != 0;
    const T* __restrict__ table = (const T*)A.table;

    if (A.mode == DSP_ALIGN_INL) {
        if constexpr (!is_float_row<IN>) {
            T* out = (T*)A.out + row * A.out_stride;
            const int p = A.table_len;
            bool range = false;
            for (int g0 = 0; g0 < row_groups<N>(n); g0 += K) {
                long long x[K][N];
                load_row_groups<long long, IN, N, K>(x, w, n, g0, lane);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    T y[N];
#pragma unroll
                    for (int j = 0; j < N; ++j) {
                        const long long code = x[k][j];
                        const bool inside = code >= 0 && code < p;  // (lanes past the row hold 0: inside, p >= 1)
                        range |= !inside;
                        // numba's and NumPy 2's typing alike: int32 + float32 is a float64 sum, rounded once by the store
                        y[j] = table_nan || !inside ? nanv : (T)((double)code + (double)table[code]);
                    }
                    store_lane<T, N, OV>(out, in_row<N>(g0, k, 0, lane), n, y);
                }
            }
            if (!table_nan && wave_any(range) && lane == 0) set_error(err, DSP_E_INL_RANGE, row);  // (inl_correction.py:51-52 returns first)
        }
        return;
    }

    if (A.mode == DSP_ALIGN_CORRECT) {
        T* out = (T*)A.out + row * A.out_stride;
        bool bad = false;
        for (int g0 = 0; g0 < row_groups<N>(n); g0 += K) {
            T x[K][N];
            load_row_groups<T, IN, N, K>(x, w, n, g0, lane);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int at = in_row<N>(g0, k, 0, lane);
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    bad |= at + j < n && x[k][j] != x[k][j];
                    if (at + j >= A.start && at + j < A.stop) x[k][j] = x[k][j] - table[at + j - A.start];
                }
                store_lane<T, N, OV>(out, at, n, x[k]);
            }
        }
        if (wave_any(bad) || table_nan) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // (the row's first stores are out of the way before other lanes write the same places)
            fill_row(out, n, nanv, lane);
        }
        return;
    }

    // ---- the two that look at the row as a whole first: the NaN rule, and the extremes with it for the centroid
    bool bad = false;
    T lo_v = (T)INFINITY, hi_v = (T)-INFINITY;
    int lo = 0x7fffffff, hi = 0x7fffffff;
    if (A.mode == DSP_ALIGN_CENTROID || is_float_row<IN>) {
        for (int g0 = 0; g0 < row_groups<N>(n); g0 += K) {
            T x[K][N];
            load_row_groups_kept<T, IN, N, K>(x, w, n, g0, lane);
#pragma unroll
            for (int k = 0; k < K; ++k)
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const int at = in_row<N>(g0, k, j, lane);
                    if (at < n) {
                        const T v = x[k][j];
                        bad |= v != v;
                        if (A.mode == DSP_ALIGN_CENTROID) {  // (a lane's indices ascend: `at` is never below what it holds)
                            if (v < lo_v || (v == lo_v && at < lo)) lo_v = v, lo = at;
                            if (v > hi_v || (v == hi_v && at < hi)) hi_v = v, hi = at;
                        }
                    }
                }
        }
        bad = wave_any(bad);
    }

    if (A.mode == DSP_ALIGN_CENTROID) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {  // the first of equal extremes wins across lanes too
            const T ov = __shfl_xor(lo_v, m);
            const int oi = __shfl_xor(lo, m);
            if (ov < lo_v || (ov == lo_v && oi < lo)) lo_v = ov, lo = oi;
            const T pv = __shfl_xor(hi_v, m);
            const int pi = __shfl_xor(hi, m);
            if (pv > hi_v || (pv == hi_v && pi < hi)) hi_v = pv, hi = pi;
        }
        T result = nanv;
        if (!bad && lo < hi) {  // (a row without a NaN has both extremes inside it; hi <= lo: undefined in the reference)
            int first_pos = 0x7fffffff, last_neg = -1;
            for (int i0 = lo; i0 < hi; i0 += 64 * U) {
                T x[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int at = i0 + u * 64 + lane;
                    x[u] = at < hi ? (T)w[at] : (T)0;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int at = i0 + u * 64 + lane;
                    if (x[u] > (T)0) first_pos = min(first_pos, at);
                    if (x[u] < (T)0) last_neg = max(last_neg, at);
                }
            }
            first_pos = wave_min(first_pos);
            last_neg = wave_max(last_neg);
            if (first_pos != 0x7fffffff && last_neg >= 0) {  // (neither: undefined in the reference)
                const double c_a = (double)first_pos + A.shift, c_b = (double)last_neg + A.shift;
                result = (T)__builtin_rint((c_a + c_b) / 2);  // round(): half to even
            }
        }
        if (lane == 0) ((T*)A.scalar_out)[row * A.scalar_stride] = result;
        return;
    }

    // ---- DSP_ALIGN_WINDOW, with or without the template behind it
    const int s = A.size;
    const T c = A.centroid ? ((const T*)A.centroid)[row * A.centroid_stride] : (T)A.centroid_const;
    AlignWindow win = {0, 0, 0, 0};
    if (!bad) {
        if (c != c) {
            if (lane == 0) set_error(err, DSP_E_ALIGN_CENTROID, row);  // wf_alignment.py:63-64, behind the row's NaN rule
        } else {
            win = dsp_align_window((double)c, A.shift, s, n);
        }
    }
    T* out = A.out ? (T*)A.out + row * A.out_stride : nullptr;
    T* out2 = A.correct ? (T*)A.out2 + row * A.out2_stride : nullptr;
    const bool nan_row = bad || win.kind == 0;
    for (int j0 = 0; j0 < s; j0 += 64 * U) {
        T x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * 64 + lane;
            // every index below lies in the row: dsp_align_window
            const int at = win.kind == 1 ? win.first + j : (win.kind == 2 ? (j < win.fill || win.count == 1 ? 0 : j - win.fill) : j);
            x[u] = j < s && !nan_row ? (T)w[at] : nanv;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * 64 + lane;
            if (j < s) {
                if (out) out[j] = x[u];
                if (out2) out2[j] = nan_row || table_nan ? nanv : (j >= A.start && j < A.stop ? x[u] - table[j - A.start] : x[u]);
            }
        }
    }
}

template <typename T, typename IN>
void launch_align(const AlignArgs* A, int64_t n_wf, int vec, int out_vec, int* err, hipStream_t stream) {
    const unsigned blocks = row_blocks(n_wf);
    if (vec && out_vec)
        hipLaunchKernelGGL((dsp_align_kernel<T, IN, RowVec<IN>::N, true>), dim3(blocks), dim3(256), 0, stream, *A, n_wf, err);
    else if (vec)
        hipLaunchKernelGGL((dsp_align_kernel<T, IN, RowVec<IN>::N, false>), dim3(blocks), dim3(256), 0, stream, *A, n_wf, err);
    else
        hipLaunchKernelGGL((dsp_align_kernel<T, IN, 1, false>), dim3(blocks), dim3(256), 0, stream, *A, n_wf, err);
}

}  // namespace

extern "C" int dsp_internal_launch_align(const AlignArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream) {
    if (n_wf <= 0) return 0;
    const int f64 = A->f64, out_vec = A->out_vec;
    // (the planner's bounds: every index the kernel forms from them lies in a row or a table)
    const bool table = A->mode == DSP_ALIGN_INL || A->mode == DSP_ALIGN_CORRECT || (A->mode == DSP_ALIGN_WINDOW && A->correct);
    const int corr_len = A->mode == DSP_ALIGN_WINDOW ? A->size : A->len;
    if (A->len < 1 || A->mode < DSP_ALIGN_INL || A->mode > DSP_ALIGN_CORRECT || (table && (!A->table || A->table_len < 1 || !A->table_nan)) ||
        (A->mode == DSP_ALIGN_INL && (!A->out || dtype == DSP_F32 || dtype == DSP_F64)) || (A->mode == DSP_ALIGN_CENTROID && !A->scalar_out) ||
        (A->mode == DSP_ALIGN_WINDOW && (A->size < 1 || A->size > A->len || (A->correct ? !A->out2 : !A->out))) || (A->mode == DSP_ALIGN_CORRECT && !A->out) ||
        ((A->mode == DSP_ALIGN_CORRECT || (A->mode == DSP_ALIGN_WINDOW && A->correct)) &&
         (A->start < 0 || A->stop > corr_len || A->start >= A->stop || A->stop - A->start > A->table_len)))
        return (int)hipErrorInvalidValue;
    if (table) {
        int* flag = const_cast<int*>(A->table_nan);
        const hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), stream);
        if (e != hipSuccess) return (int)e;
        const unsigned blocks = (unsigned)((A->table_len + 1023) / 1024 > 64 ? 64 : (A->table_len + 1023) / 1024);
        if (f64)
            hipLaunchKernelGGL(dsp_align_table_kernel<double>, dim3(blocks), dim3(256), 0, stream, (const double*)A->table, A->table_len, flag);
        else
            hipLaunchKernelGGL(dsp_align_table_kernel<float>, dim3(blocks), dim3(256), 0, stream, (const float*)A->table, A->table_len, flag);
    }
    if (f64) {
        switch (dtype) {
            case DSP_I16: launch_align<double, int16_t>(A, n_wf, vec, out_vec, err, stream); break;
            case DSP_U16: launch_align<double, uint16_t>(A, n_wf, vec, out_vec, err, stream); break;
            case DSP_I32: launch_align<double, int32_t>(A, n_wf, vec, out_vec, err, stream); break;
            case DSP_U32: launch_align<double, uint32_t>(A, n_wf, vec, out_vec, err, stream); break;
            default: launch_align<double, double>(A, n_wf, vec, out_vec, err, stream); break;
        }
    } else {
        switch (dtype) {
            case DSP_I16: launch_align<float, int16_t>(A, n_wf, vec, out_vec, err, stream); break;
            case DSP_U16: launch_align<float, uint16_t>(A, n_wf, vec, out_vec, err, stream); break;
            case DSP_I32: launch_align<float, int32_t>(A, n_wf, vec, out_vec, err, stream); break;
            case DSP_U32: launch_align<float, uint32_t>(A, n_wf, vec, out_vec, err, stream); break;
            default: launch_align<float, float>(A, n_wf, vec, out_vec, err, stream); break;
        }
    }
    return (int)hipGetLastError();
}
