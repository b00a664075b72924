// dsp_thresh.hip -- multi_time_point_thresh (processors/time_point_thresh.py:225-401): the times at which a row crosses m thresholds, found
// from one starting sample; and time_over_threshold (processors/time_over_threshold.py:11-48): the number of samples above a threshold.
//
// A wavefront per row, four to a workgroup, nothing in LDS.
//   pass 1   the row is streamed through registers (dsp_row_stream.h: 16 bytes per lane and load, four loads in flight; a sample per lane,
//            eight in flight, where start, stride or length are not whole 16-byte vectors): "a NaN" of the row, which both processors need, and the
//            count of samples above the threshold, which is time_over_threshold whole.
//   ranking  a threshold per lane (m <= 64); its rank is the number of thresholds below it (or equal with a lower index); one
//            forward permute puts thresholds and their indices in ascending order, one per lane.  The first one >= w[t_start] splits them.
//   pass 2   the reference's two walks, 64 samples a step.  The upper walk goes from t_start with the polarity and takes the thresholds
//            upwards, the lower walk from t_start - 1 against it and takes them downwards; the test is w[i] <= thr < w[i + pol] in both.
//            A step looks at 64 positions for the current threshold: a hit (ballot, first lane) gives that threshold its time and makes the
//            next one current WITHOUT moving -- the next step starts at the hit --, no hit moves the window on: at most n / 64 + m steps.
//            The thresholds are a chain: one that is never crossed blocks all behind it, and the position never goes back
//            (tests/threshold_cases.py has the rows on which m independent walks give something else).
//            Negative indices wrap as NumPy's do: with polarity < 0 the upper walk reads w[-1] at i = 0, and from t_start = 0 the lower
//            walk starts at i = -1 and reads w[-1] and w[-2]; the times -1, -2, -0.5 are the reference's.  No read leaves the row:
//            0 <= t_start < n is checked first (the row is a NaN row otherwise), n >= 2 by the planner.
//            The row was just read: the walks find it in the caches.
//   times    a result per lane, in ascending order of the thresholds; lane r writes t_out[index of the r-th smallest].
#include <hip/hip_runtime.h>

#include "dsp_launch.h"
#include "dsp_row_stream.h"
#include "dsp_wave.h"

namespace {

// the time of a crossing between w[i] = wi and w[i + pol] = wn (time_point_thresh.py:335-358)
template <typename T>
__device__ __forceinline__ T crossing_time(int mode, int pol, int i, T wi, T wn, T thr) {
    switch (mode) {
        case 'i': return (T)i;
        case 'a':
        case 'f': return (T)(pol < 0 ? i : i + 1);
        case 'b':
        case 'c': return (T)(pol > 0 ? i : i - 1);
        case 'r': return (T)((thr - wi < wn - thr) ? i : i + pol);
        case 'n': return (T)((double)i + 0.5 * (double)pol);
        default: return (T)i + (thr - wi) / (wn - wi);  // 'l' (the sum in the loop's type: exact integers up to the planner's 2^24 samples)
    }
}

// N: samples per lane and load (1, or those of a 16-byte vector: rows then start on 16-byte boundaries and hold whole vectors)
template <typename T, typename IN, int N>
__global__ void __launch_bounds__(256) dsp_thresh_kernel(ThreshArgs A, int64_t n_wf, int* err) {
    constexpr int K = N > 1 ? 4 : 8;  // loads in flight
    const int lane = lane_id();
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_wf) return;  // (whole wavefronts: no barrier in this kernel)
    const IN* w = (const IN*)A.wf + row * A.wf_stride + A.wf_offset;
    const int n = A.len, m = A.m;
    const T nanv = quiet_nan<T>();
    // time_over_threshold's threshold (multi_time_point_thresh counts nothing)
    const T above = m == 0 ? (A.thr ? ((const T*)A.thr)[row * A.thr_stride] : (T)A.thr_const) : (T)0;

    // pass 1
    bool bad = false;
    int count = 0;
    for (int g0 = 0; g0 < row_groups<N>(n); g0 += K) {
        T x[K][N];
        load_row_groups<T, IN, N, K>(x, w, n, g0, lane);
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const T v = x[k][j];
                const bool in = in_row<N>(g0, k, j, lane) < n;
                bad |= in && v != v;
                count += (in && v > above) ? 1 : 0;
            }
    }
    bad = wave_any(bad);

    if (m == 0) {  // time_over_threshold
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) count += __shfl_xor(count, s);
        if (lane == 0) ((T*)A.out)[row * A.out_stride] = (bad || above != above) ? nanv : (T)count;
        return;
    }

    // multi_time_point_thresh
    T* out = (T*)A.out + row * A.out_stride;
    const T* list = (const T*)A.thr + row * A.thr_stride + A.thr_offset;
    const T thr = lane < m ? list[lane] : (T)__builtin_huge_valf();
    const T ts_f = A.ts ? ((const T*)A.ts)[row * A.ts_stride] : (T)A.ts_const;
    // (the reference's order: any NaN, then the range of t_start -- before w[t_start] is touched)
    if (bad || wave_any(thr != thr) || ts_f != ts_f || ts_f < (T)0 || ts_f >= (T)n) {
        if (lane < m) out[lane] = nanv;
        return;
    }
    const int ts = (int)ts_f;
    const int pol = A.polarity, mode = A.mode;
    auto at = [&](int j) -> T { return (T)w[j < 0 ? j + n : j]; };  // (j >= -2, n >= 2)
    const T a_start = (T)w[ts];

    // rank: thresholds below this one, or equal with a lower index (lanes without a threshold keep their own place)
    int rank = 0;
    for (int k = 0; k < m; ++k) {
        const T tk = readlane(thr, k);
        rank += (tk < thr || (tk == thr && k < lane)) ? 1 : 0;
    }
    rank = lane < m ? rank : lane;
    const T sorted = wave_send(thr, rank);      // the thresholds in ascending order, one per lane
    const int index = wave_send(lane, rank);    // ... and where each stands in the list
    const int i_start = __builtin_popcountll(__ballot(lane < m && thr < a_start));  // the first sorted threshold >= a_start

    T res = nanv;  // the time of the lane's threshold (in sorted order)
    // a walk over i in [lo, hi] from i0 in steps of dir, thresholds from tp in steps of tdir
    auto walk = [&](int i0, int dir, int lo, int hi, int tp, int tdir) {
        int base = i0;
        while (tp >= 0 && tp < m && base >= lo && base <= hi) {
            const T cur = readlane(sorted, uniform(tp));
            const int i = base + dir * lane;
            const bool live = i >= lo && i <= hi;
            T wi = (T)0, wn = (T)0;
            if (live) {
                wi = at(i);
                wn = at(i + pol);
            }
            const unsigned long long hits = __ballot(live && wi <= cur && cur < wn);
            if (hits) {
                const int first = __builtin_ctzll(hits);
                const T t = __shfl(crossing_time<T>(mode, pol, i, wi, wn, cur), first);
                res = lane == tp ? t : res;
                tp += tdir;
                base += dir * first;  // (the next threshold is looked for from the same sample on)
            } else {
                base += dir * 64;
            }
        }
    };
    if (pol > 0) {
        walk(ts, 1, ts, n - 2, i_start, 1);
        walk(ts - 1, -1, 0, ts - 1, i_start - 1, -1);
    } else {
        walk(ts, -1, 0, ts, i_start, 1);
        walk(ts - 1, 1, ts - 1, n - 2, i_start - 1, -1);
    }
    if (lane < m) out[index] = res;
}

template <typename T, typename IN>
void launch_thresh(const ThreshArgs* A, int64_t n_wf, int vec, int* err, hipStream_t stream) {
    const unsigned blocks = row_blocks(n_wf);
    if (vec)
        hipLaunchKernelGGL((dsp_thresh_kernel<T, IN, RowVec<IN>::N>), dim3(blocks), dim3(256), 0, stream, *A, n_wf, err);
    else
        hipLaunchKernelGGL((dsp_thresh_kernel<T, IN, 1>), dim3(blocks), dim3(256), 0, stream, *A, n_wf, err);
}

}  // namespace

extern "C" int dsp_internal_launch_thresh(const ThreshArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream) {
    if (n_wf <= 0) return 0;
    // (the planner's bounds: a threshold per lane; the wrapped reads w[-1], w[-2] stay inside a row of two samples or more)
    if (A->m < 0 || A->m > DSP_THRESH_MAX || A->len < 1 || (A->m > 0 && (A->len < 2 || !A->thr || (A->polarity != 1 && A->polarity != -1))))
        return (int)hipErrorInvalidValue;
    switch (dtype) {
        case DSP_F32: launch_thresh<float, float>(A, n_wf, vec, err, stream); break;
        case DSP_I16: launch_thresh<float, int16_t>(A, n_wf, vec, err, stream); break;
        case DSP_U16: launch_thresh<float, uint16_t>(A, n_wf, vec, err, stream); break;
        default: launch_thresh<double, double>(A, n_wf, vec, err, stream); break;
    }
    return (int)hipGetLastError();
}
