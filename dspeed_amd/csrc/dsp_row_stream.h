// dsp_row_stream.h -- how a wavefront streams a row from memory through its registers: shared by the kernels that give a row to a wavefront,
// four rows to a workgroup (dsp_reduce.hip, dsp_thresh.hip, dsp_hist.hip, dsp_extrema.hip; dsp_spectrum.hip and dsp_sort.hip stage rows into LDS
// through the same loader, a wavefront or the four wavefronts of a workgroup per row).  Internal header.
//
// A row of n samples is read in groups of 64 N: lane l holds samples [g 64 N + l N, + N) of group g.  N is the number of samples in 16
// bytes (RowVec) where row starts, stride and length are whole 16-byte vectors -- the planner's rule and the pointer's alignment: `vec` of
// the launchers --, and 1 otherwise.  K groups are requested before the first is looked at.  A kernel of this kind loops
//     for (int g0 = 0; g0 < row_groups<N>(n); g0 += K) { T x[K][N]; load_row_groups<T, IN, N, K>(x, w, n, g0, lane); ... in_row<N>(g0, k, j, lane) < n ... }
// and launches row_blocks(n_wf) workgroups of 256 with N = vec ? RowVec<IN>::N : 1.
// dsp_thresh.hip does (its code is the one it had with a loop of its own, instruction for instruction).  dsp_reduce.hip, dsp_hist.hip and
// dsp_extrema.hip share RowVec and row_blocks and keep the loops they were tuned with: through load_row_groups the same loads cost
// dsp_reduce_kernel<float, true> and dsp_hist_kernel<double, double, 2> registers, the latter a wavefront per SIMD, and left to the
// inliner they cost the peak finder up to 40 % of its rate (profiles/r11_row_stream.md).
#pragma once
#include <hip/hip_runtime.h>

namespace {

template <typename IN>
struct RowVec;  // 16 bytes of a row
#define DSP_ROW_VEC(IN, ELEM, COUNT)                                \
    template <>                                                     \
    struct RowVec<IN> {                                             \
        static constexpr int N = COUNT;                             \
        typedef ELEM vec __attribute__((ext_vector_type(COUNT)));   \
    }
DSP_ROW_VEC(float, float, 4);
DSP_ROW_VEC(int16_t, short, 8);
DSP_ROW_VEC(uint16_t, unsigned short, 8);
DSP_ROW_VEC(double, double, 2);
DSP_ROW_VEC(int32_t, int, 4);
DSP_ROW_VEC(uint32_t, unsigned int, 4);
#undef DSP_ROW_VEC

template <int N>
__device__ __forceinline__ int row_groups(int n) {
    return (n + 64 * N - 1) / (64 * N);
}

// where element (k, j) of the groups loaded from g0 on stands in the row; >= n: past the row
template <int N>
__device__ __forceinline__ int in_row(int g0, int k, int j, int lane) {
    return (g0 + k) * (64 * N) + lane * N + j;
}

// x[k][j] = sample in_row(g0, k, j) as a T, for groups g0 .. g0 + K - 1; lanes past the end of the row read nothing and hold 0.  The loads are
// non-temporal: the row is not read again.
template <typename T, typename IN, int N, int K>
__device__ __forceinline__ void load_row_groups(T (&x)[K][N], const IN* w, int n, int g0, int lane) {
    if constexpr (N > 1) {
        // n is a multiple of N: a vector that starts inside the row lies inside it whole
        typedef typename RowVec<IN>::vec vec;
        const vec* wv = (const vec*)w;
        vec v[K] = {};
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (in_row<N>(g0, k, 0, lane) < n) v[k] = __builtin_nontemporal_load(wv + ((g0 + k) * 64 + lane));
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

}  // namespace

// workgroups of a launch: a wavefront per row, four to a workgroup
static inline unsigned row_blocks(int64_t n_wf) { return (unsigned)((n_wf + 3) / 4); }
