// dsp_hist.hip -- histogram (processors/histogram.py:14-89) and histogram_stats (processors/histogram_stats.py:157-261): the histogram of a
// row between its own extremes, and the mode, its left edge and the half width at half maximum read off a histogram.  The first
// scatter-shaped workload here: a pass for the row's extremes, a second with a data-dependent increment per sample.
//
// A wavefront per row, four to a workgroup, rows dealt out workgroup by workgroup; the row is streamed as dsp_row_stream.h lays it out (16
// bytes per lane and load, four loads in flight; a sample per lane where start, stride or length are not whole 16-byte vectors).
//   pass 1   minimum, maximum, "a NaN" of the row: per lane, then one exchange across the wavefront.  Pass 2 reads the row again, past the caches this
//            time: keeping a short row (four groups of loads, 1024 float32 samples) in registers instead measured 6 - 7 % slower at either
//            length, the choice costing every row (-DDSP_HIST_KEEP builds it; profiles/r08_histogram.md).
//   borders  b[i] = min + i * delta, b[m] = max, delta = (max - min) / m -- formed in float64 and rounded once into the loop's type: for the
//            float64 loop the reference body as written, for the float32 loop what numba's typing makes of it (float32 / int64 is float64,
//            and so is np.linspace); tests/histogram_cases.py has both rule sets spelled out.
//   pass 2   every sample other than the maximum: k = floor((w - min) / delta) with w - min rounded in the loop's type and the division in
//            float64; 1 is added to counter k of the wavefront's own LDS region with a no-return LDS atomic.  k >= m (the quotient of the
//            largest samples below the maximum may round up to m) is dropped: the reference stores past the end of weights_out there.
//   epilogue weights (the counters, exact in the loop's type: the planner bounds the row length) and borders, where the program stores
//            them; histogram_stats on the counters and borders the wavefront still holds, a bin per lane and round: the mode as the first
//            occurrence of the largest weight (or the edge nearest max_in), the two searches for the half maximum as ballots.
// The four wavefronts of a workgroup share nothing: no workgroup barrier.  A wavefront's LDS instructions execute in issue order, so the
// clearing of the counters, the increments and the reads of the epilogue need a compiler fence only (wave_sync).
// A NaN in the row: weights 0, borders NaN (reference lines 64-68); so for an infinite sample, where the reference converts a NaN to an
// integer.  A constant row: delta 0, borders all equal, weights 0 (lines 80-81).
// dsp_hist_stats_kernel is histogram_stats alone, weights and edges read from rows in memory: the same device function.
#include <hip/hip_runtime.h>

#include "dsp_kernels.h"
#include "dsp_launch.h"
#include "dsp_row_stream.h"
#include "dsp_wave.h"

namespace {

__device__ __forceinline__ float absv(float v) { return __builtin_fabsf(v); }
__device__ __forceinline__ double absv(double v) { return __builtin_fabs(v); }

// (value, index) across the wavefront: the better value, the lower index between equals.  GREATER: the largest value wins, else the smallest.
// A NaN never wins against a number and keeps its place against a NaN (every comparison is false).
template <bool GREATER, typename T>
__device__ __forceinline__ int wave_first_best(T v, int i) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const T ov = __shfl_xor(v, s);
        const int oi = __shfl_xor(i, s);
        const bool take = (GREATER ? ov > v : ov < v) || (ov == v && oi < i);
        v = take ? ov : v;
        i = take ? oi : i;
    }
    return uniform(i);
}

// histogram_stats.py:220-261 on m weights wt(i) and m + 1 edges ed(i), a bin per lane and round.  CHECK_NAN: the weights come from memory.
template <bool CHECK_NAN, typename T, typename WF, typename EF>
__device__ __forceinline__ void hist_stats(int m, T max_in, WF wt, EF ed, int lane, T& mode_out, T& max_out, T& fwhm_out) {
    mode_out = max_out = fwhm_out = quiet_nan<T>();
    if (CHECK_NAN) {
        bool nan = false;
        for (int i = lane; i < m; i += 64) {
            const T w = wt(i);
            nan |= w != w;
        }
        if (wave_any(nan)) return;
    }
    // the mode: the first of the largest weights (strict comparisons from bin 0 on), or the edge nearest max_in by the two branches
    int idx;
    if (max_in != max_in) {
        T bv = wt(0);
        int bi = 0;
        for (int i = lane; i < m; i += 64) {
            const T w = wt(i);
            const bool better = w > bv;
            bv = better ? w : bv;
            bi = better ? i : bi;
        }
        idx = wave_first_best<true>(bv, bi);
    } else if (max_in > ed(m - 1)) {
        idx = m - 1;
    } else {
        T bv = absv(max_in - ed(0));  // (a NaN here -- NaN edges -- and nothing is nearer: bin 0, as the reference's comparisons leave it)
        int bi = 0;
        for (int i = lane; i < m; i += 64) {
            const T d = absv(max_in - ed(i));
            const bool better = d < bv;
            bv = better ? d : bv;
            bi = better ? i : bi;
        }
        idx = wave_first_best<false>(bv, bi);
    }
    mode_out = (T)idx;
    const T edge = ed(idx);
    max_out = edge;
    const double half = 0.5 * (double)wt(idx);
    T fwhm = quiet_nan<T>();
    // upwards from the mode: the first bin at or below the half maximum that is not empty
    for (int base = idx & ~63; base < m; base += 64) {
        const int i = base + lane;
        const T w = i < m ? wt(i) : (T)0;
        const unsigned long long hit = __ballot(i >= idx && i < m && (double)w <= half && w != (T)0);
        if (hit) {
            fwhm = absv(edge - ed(base + __builtin_ctzll(hit)));
            break;
        }
    }
    // below the mode, from bin 0 upwards: the first bin at or above it that is not empty; it counts only if it lies further out (a fwhm that
    // is still NaN stays NaN: NaN < x is false)
    for (int base = 0; base < idx; base += 64) {
        const int i = base + lane;
        const T w = i < idx ? wt(i) : (T)0;
        const unsigned long long hit = __ballot(i < idx && (double)w >= half && w != (T)0);
        if (hit) {
            const T other = absv(edge - ed(base + __builtin_ctzll(hit)));
            fwhm = fwhm < other ? other : fwhm;
            break;
        }
    }
    fwhm_out = fwhm;
}

template <typename T>
__device__ __forceinline__ void store_stats(const HistArgs& A, int64_t row, int lane, T mode, T mx, T fwhm) {
    if (lane != 0) return;
    const T v[3] = {mode, mx, fwhm};
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (A.s_out[k]) ((T*)A.s_out[k])[row * A.s_stride[k]] = v[k];
}

template <typename T>
__device__ __forceinline__ T max_in_of(const HistArgs& A, int64_t row) {
    return A.max_in ? ((const T*)A.max_in)[row * A.max_in_stride] : (T)A.max_in_const;
}

// N: samples per lane and load (1, or those of a 16-byte vector: rows then start on 16-byte boundaries and hold whole vectors)
template <typename T, typename IN, int N>
__global__ void __launch_bounds__(256) dsp_hist_kernel(HistArgs A, int64_t n_wf, int* err) {
    extern __shared__ uint32_t hist_counters[];  // [4][mp]: a region per wavefront
    typedef typename RowVec<IN>::vec vec;
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const int n = A.len, m = A.m, mp = (m + 63) & ~63;
    uint32_t* cnt = hist_counters + wave * mp;
    const int per_group = 64 * N, n_groups = (n + per_group - 1) / per_group;
#ifdef DSP_HIST_KEEP
    const bool keep = n_groups <= 4;  // (the A/B of tools/histogram_rate.py: a short row stays in registers between the passes)
#else
    const bool keep = false;  // every row is read twice
#endif
    // (whole wavefronts, a different number of rows each: no barrier in this kernel)
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < n_wf; row += (int64_t)gridDim.x * 4) {
        const IN* w = (const IN*)A.wf + row * A.wf_stride + A.wf_offset;
        for (int i = lane; i < mp; i += 64) cnt[i] = 0u;
        T x[4][N];
        // samples [g * 64 N + lane * N, + N) of group g, four groups requested before the first is looked at; `stream`: past the caches
        auto load = [&](int g0, bool stream) {
            if constexpr (N > 1) {
                const vec* wv = (const vec*)w;
                vec v[4] = {};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int at = (g0 + k) * per_group + lane * N;
                    if (at < n) v[k] = stream ? __builtin_nontemporal_load(wv + ((g0 + k) * 64 + lane)) : wv[(g0 + k) * 64 + lane];  // (whole vectors: dsp_row_stream.h)
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int j = 0; j < N; ++j) x[k][j] = (T)v[k][j];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int at = (g0 + k) * 64 + lane;
                    x[k][0] = at < n ? (T)w[at] : (T)0;
                }
            }
        };
        // pass 1
        T mn = (T)w[0], mx = mn;
        bool bad = false;
        for (int g0 = 0; g0 < n_groups; g0 += 4) {
            load(g0, keep);
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const T v = x[k][j];
                    const bool in = (g0 + k) * per_group + lane * N + j < n;
                    bad |= in && v != v;
                    mn = in && v < mn ? v : mn;
                    mx = in && v > mx ? v : mx;
                }
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const T on = __shfl_xor(mn, s), ox = __shfl_xor(mx, s);
            mn = on < mn ? on : mn;
            mx = ox > mx ? ox : mx;
        }
        bad = wave_any(bad) || __builtin_isinf(mn) || __builtin_isinf(mx);
        const double delta = (double)(T)(mx - mn) / (double)m;
        // pass 2
        wave_sync();
        if (!bad && delta != 0.0) {
            for (int g0 = 0; g0 < n_groups; g0 += 4) {
                if (!keep) load(g0, true);
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int j = 0; j < N; ++j) {
                        const T v = x[k][j];
                        const bool in = (g0 + k) * per_group + lane * N + j < n;
                        const double q = (double)(T)(v - mn) / delta;
                        const bool counts = in && v != mx && q < (double)m;  // (q >= 0: its floor is its integer part)
#ifndef DSP_HIST_NO_COMBINE  // (the A/B of tools/histogram_rate.py)
                        // lanes that all hit one bin (a quiet baseline: whole groups of samples) add once: 64 same-address increments serialise,
                        // 2.65 ms against 1.37 per 131 072 pulse rows of 8192 samples (profiles/r08_histogram.md); up to 7 % dearer on rows spread over the bins
                        const int k = counts ? (int)q : -1;
                        const int k0 = uniform(k);
                        if (__ballot(k != k0) == 0ull) {
                            if (k0 >= 0 && lane == 0) atomicAdd(&cnt[k0], 64u);
                        } else if (counts) {
                            atomicAdd(&cnt[k], 1u);
                        }
#else
                        if (counts) atomicAdd(&cnt[(int)q], 1u);  // (result unused: ds_add_u32)
#endif
                    }
            }
        }
        wave_sync();
        auto border = [&](int i) -> T { return bad ? quiet_nan<T>() : (i == m ? mx : (T)((double)mn + (double)i * delta)); };
        if (A.w_out) {
            T* out = (T*)A.w_out + row * A.w_stride;
            for (int i = lane; i < m; i += 64) out[i] = (T)cnt[i];
        }
        if (A.b_out) {
            T* out = (T*)A.b_out + row * A.b_stride;
            for (int i = lane; i <= m; i += 64) out[i] = border(i);
        }
        if (A.stats) {
            T mode, edge, fwhm;
            hist_stats<false, T>(m, max_in_of<T>(A, row), [&](int i) -> T { return (T)cnt[i]; }, border, lane, mode, edge, fwhm);
            store_stats<T>(A, row, lane, mode, edge, fwhm);
        }
        wave_sync();  // (the next row's clearing stays behind these reads)
    }
}

template <typename T>
__global__ void __launch_bounds__(256) dsp_hist_stats_kernel(HistArgs A, int64_t n_wf, int* err) {
    const int lane = lane_id();
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n_wf; row += (int64_t)gridDim.x * 4) {
        const T* wt = (const T*)A.w_in + row * A.w_in_stride + A.w_in_offset;
        const T* ed = (const T*)A.e_in + row * A.e_in_stride + A.e_in_offset;
        T mode, edge, fwhm;
        hist_stats<true, T>(A.m, max_in_of<T>(A, row), [&](int i) -> T { return wt[i]; }, [&](int i) -> T { return ed[i]; }, lane, mode, edge, fwhm);
        store_stats<T>(A, row, lane, mode, edge, fwhm);
    }
}

// rows are dealt out to at most this many workgroups: 8192, or the program's own cap (DSP_OP_HISTOGRAM ip[1])
unsigned hist_blocks(int64_t n_wf, int32_t max_blocks = 0) {
    const int64_t cap = max_blocks >= 1 && max_blocks < 8192 ? max_blocks : 8192;
    const int64_t blocks = row_blocks(n_wf);
    return (unsigned)(blocks < cap ? blocks : cap);
}

template <typename T, typename IN>
void launch_hist(const HistArgs* A, int64_t n_wf, int vec, int* err, hipStream_t stream) {
    const unsigned lds = (unsigned)dsp_hist::lds_bytes(A->m);
    if (vec)
        hipLaunchKernelGGL((dsp_hist_kernel<T, IN, RowVec<IN>::N>), dim3(hist_blocks(n_wf, A->max_blocks)), dim3(256), lds, stream, *A, n_wf, err);
    else
        hipLaunchKernelGGL((dsp_hist_kernel<T, IN, 1>), dim3(hist_blocks(n_wf, A->max_blocks)), dim3(256), lds, stream, *A, n_wf, err);
}

}  // namespace

extern "C" int dsp_internal_launch_hist(const HistArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream) {
    if (n_wf <= 0) return 0;
    if (A->m < 1 || A->m > DSP_HIST_MAX_BINS) return (int)hipErrorInvalidValue;  // (the planner's bound: the counters' LDS)
    if (!A->wf) {
        if (dtype == DSP_F64)
            hipLaunchKernelGGL((dsp_hist_stats_kernel<double>), dim3(hist_blocks(n_wf)), dim3(256), 0, stream, *A, n_wf, err);
        else
            hipLaunchKernelGGL((dsp_hist_stats_kernel<float>), dim3(hist_blocks(n_wf)), dim3(256), 0, stream, *A, n_wf, err);
        return (int)hipGetLastError();
    }
    switch (dtype) {
        case DSP_F32: launch_hist<float, float>(A, n_wf, vec, err, stream); break;
        case DSP_I16: launch_hist<float, int16_t>(A, n_wf, vec, err, stream); break;
        case DSP_U16: launch_hist<float, uint16_t>(A, n_wf, vec, err, stream); break;
        default: launch_hist<double, double>(A, n_wf, vec, err, stream); break;
    }
    return (int)hipGetLastError();
}
