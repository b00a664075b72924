// dsp_pulses.hip -- the pulse picker of the SiPM recipes, the two steps behind the peak finder's candidate list:
//   peak_snr_threshold (processors/peak_snr_threshold.py:19-71): of the candidates of a row those whose neighbourhood goes down far enough
//   multi_a_filter (processors/multi_a_filter.py:20-57): the row's amplitudes at the positions of a list
// apart or in one launch, where the pick-off reads the packed list from registers.
//
// A wavefront per row, four to a workgroup, nothing in LDS (dsp_thresh.hip's geometry).
//   pass 1   ONLY with multi_a_filter in the launch: the row is streamed through registers (dsp_row_stream.h) for "a NaN in the row", which
//            makes its amplitudes NaN.  The picker has no such rule (peak_snr_threshold.py never looks at the row as a whole) and needs m
//            windows of 2 width samples, not n: alone it reads those and nothing else.
//   picking  a candidate per lane (m <= 64).  The lane walks its window [a, b) (dsp_kernels.h, dsp_pulses: b is never looked at) in
//            ascending j with the reference's strict comparison from min_index = a, so the first of tied minima wins, a NaN sample never
//            takes the minimum and an empty window leaves a.  The addresses do not depend on the data: U loads are in flight before the
//            first comparison, and the samples at a and at c with them.  Reads go to memory; behind pass 1 they find the row in the
//            caches, without it they are the only traffic.
//   packing  the keep decision is a ballot; a kept candidate's place is the number of kept lanes below it, the others go behind them: one
//            forward permute packs the list, lanes from the count on hold NaN, lane 0 writes the count.
//   pick-off lane j reads w[int(vt[j])] for a whole number inside the row, NaN for a NaN or a position outside it; anything else is the
//            reference's DSPFatal: the error word, with the row.
// Where the reference defines no result (a candidate that is infinite or whose int() is outside the row; w[c] == 0): dsp_kernels.h and
// DESIGN.md -- dropped, no sample read; IEEE division, |x / 0| is inf or NaN and neither is below a ratio.
#include <hip/hip_runtime.h>

#include "dsp_kernels.h"
#include "dsp_launch.h"
#include "dsp_row_stream.h"
#include "dsp_wave.h"

namespace {

using namespace dsp_pulses;

// N: samples per lane and load of pass 1 (1, or those of a 16-byte vector: rows then start on 16-byte boundaries and hold whole vectors)
template <typename T, typename IN, int N>
__global__ void __launch_bounds__(256) dsp_pulses_kernel(PulsesArgs A, int64_t n_wf, int* err) {
    constexpr int K = N > 1 ? 4 : 8;  // loads in flight, pass 1
    constexpr int U = 16;             // loads in flight, a lane's window
    const int lane = lane_id();
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_wf) return;  // (whole wavefronts: no barrier in this kernel)
    const IN* __restrict__ w = (const IN*)A.wf + row * A.wf_stride + A.wf_offset;
    const int n = A.len, m = A.m;
    const T nanv = quiet_nan<T>();

    // pass 1
    bool bad = false;
    if (A.amp) {
        for (int g0 = 0; g0 < row_groups<N>(n); g0 += K) {
            T x[K][N];
            load_row_groups<T, IN, N, K>(x, w, n, g0, lane);
#pragma unroll
            for (int k = 0; k < K; ++k)
#pragma unroll
                for (int j = 0; j < N; ++j) bad |= in_row<N>(g0, k, j, lane) < n && x[k][j] != x[k][j];
        }
        bad = wave_any(bad);
    }

    const T* list = (const T*)A.list + row * A.list_stride + A.list_offset;
    T vt = lane < m ? list[lane] : nanv;  // the lane's entry: a candidate, then a position

    if (A.pick) {
        const T ratio = A.ratio ? ((const T*)A.ratio)[row * A.ratio_stride] : (T)A.ratio_const;
        bool keep = false;
        if (lane < m && !dropped((double)vt, n)) {
            const Window win = window((double)vt, n, A.width);  // 0 <= a <= c <= b <= n - 1: every j in [a, b) is in the row
            const T at_c = (T)w[win.c];
            T lowest = (T)w[win.a];  // w[min_index], min_index = a
            for (int j0 = win.a; j0 < win.b; j0 += U) {
                T x[U];
                // (past the window's end the last sample of it once more: the same value again changes nothing under a strict comparison)
#pragma unroll
                for (int u = 0; u < U; ++u) x[u] = (T)w[j0 + u < win.b ? j0 + u : win.b - 1];
#pragma unroll
                for (int u = 0; u < U; ++u) lowest = x[u] < lowest ? x[u] : lowest;  // (strict: the first occurrence stays; a NaN never enters)
            }
            const T q = lowest / at_c;
            keep = (q < (T)0 ? -q : q) < ratio;  // (a NaN quotient or ratio: not kept)
        }
        const unsigned long long kept = __ballot(keep), below = (1ull << lane) - 1ull;
        const int count = __builtin_popcountll(kept);
        const int to = keep ? __builtin_popcountll(kept & below) : count + __builtin_popcountll(~kept & below);  // a permutation of the lanes
        const T packed = wave_send(vt, to);
        vt = lane < count ? packed : nanv;
        if (A.idx_out && lane < m) ((T*)A.idx_out)[row * A.idx_stride + lane] = vt;
        if (lane == 0) A.n_out[row * A.n_stride] = (unsigned)count;
    }

    if (A.amp && lane < m) {
        T a = nanv;
        // fixed_time_pickoff.py:68-85 with mode 'i' (the position against the integer n - 1: in float64, as numba compares them)
        if (!bad && vt == vt && !(vt < (T)0) && !((double)vt > (double)(n - 1))) {
            const int i = (int)vt;
            if ((T)i == vt) {
                a = (T)w[i];
            } else if (atomicCAS(&err[0], 0, DSP_E_FTP_INT) == 0) {
                err[1] = (int)(row & 0xffffffffll);
                err[2] = (int)(row >> 32);
            }
        }
        ((T*)A.amp_out)[row * A.amp_stride + lane] = a;
    }
}

template <typename T, typename IN>
void launch_pulses(const PulsesArgs* A, int64_t n_wf, int vec, int* err, hipStream_t stream) {
    const unsigned blocks = row_blocks(n_wf);
    if (vec)
        hipLaunchKernelGGL((dsp_pulses_kernel<T, IN, RowVec<IN>::N>), dim3(blocks), dim3(256), 0, stream, *A, n_wf, err);
    else
        hipLaunchKernelGGL((dsp_pulses_kernel<T, IN, 1>), dim3(blocks), dim3(256), 0, stream, *A, n_wf, err);
}

}  // namespace

extern "C" int dsp_internal_launch_pulses(const PulsesArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream) {
    if (n_wf <= 0) return 0;
    // (the planner's bounds: an entry per lane; a width within the row; every output the ops of the launch write)
    if (A->m < 1 || A->m > DSP_PEAKS_MAX || A->len < 1 || !A->list || (!A->pick && !A->amp) || A->width < 0 || A->width > A->len ||
        (A->pick && !A->n_out) || (A->amp && (!A->amp_out || A->m >= A->len)) || (!A->amp && !A->idx_out))
        return (int)hipErrorInvalidValue;
    switch (dtype) {
        case DSP_F32: launch_pulses<float, float>(A, n_wf, vec, err, stream); break;
        case DSP_I16: launch_pulses<float, int16_t>(A, n_wf, vec, err, stream); break;
        case DSP_U16: launch_pulses<float, uint16_t>(A, n_wf, vec, err, stream); break;
        default: launch_pulses<double, double>(A, n_wf, vec, err, stream); break;
    }
    return (int)hipGetLastError();
}
