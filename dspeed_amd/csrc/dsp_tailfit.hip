// dsp_tailfit.hip -- the tail-quality chain of the Ge recipes, one waveform per LANE:
//   log_check (processors/log_check.py:11-48): the logarithm of a row that is positive throughout, NaNs otherwise,
//   poly_fit(length, deg) (processors/poly_fit.py:12-71): float64 moments of the row, one small matrix product,
//   poly_diff, poly_exp_rms (processors/poly_fit.py:74-141): two sums that round to the loop's type after every sample,
// apart, or log_check -> poly_fit in one pass, or log_check -> poly_fit -> the residuals in two passes over the same rows.
//
// The residuals add into outputs of the loop's type in place, so "mean" and rms round after every sample, and the moments are float64 sums
// in the order of the samples: a row's samples cannot be shared out among lanes without changing bits.  So -- as in dsp_fit.hip and
// dsp_pileup.hip -- the 64 lanes of a wavefront run 64 rows' chains, and the rows pass through the pile-up kernel's LDS tile
// (dsp_lane_tiles.h).  What does not vary with the row is formed once: the inverted matrix on the host, and float64(i**j) -- the exact
// integer converted once, as numba types i**j -- once per tile, a sample's powers by one lane, into an LDS table that every lane reads
// at the same entry (a broadcast).
//
// numba's typing is the rule (-ffp-contract=off: no fused multiply-add):
//   log_check    log in the loop's type (the float32 loop's through the float64 log, rounded once);
//   poly_fit     arr[j] += float64(w[i]) * float64(i**j), ascending i; out[k] = sum_j inv[k][j] * arr[j], ascending j, rounded once;
//   residuals    temp = sum_j float64(p[j]) * float64(i**j), ascending j; r = float64(w[i]) - temp  or  - exp(temp);
//                mean = T(float64(mean) + r / float64(i + 1)); rms = T(float64(rms) + r * r); at the end rms = sqrt(T(float64(rms) / float64(n - 1))).
// A row with a NaN (log_check: or a sample <= 0) is known only when the lane has been through it: the flags are carried along, a logged
// row that turns out bad is written over with NaNs behind the last tile, a fit of such a row gives NaN coefficients, and NaN coefficients
// give NaN residuals.  In the launch with all three the fitted coefficients are used as stored, rounded to the loop's type, and the second
// pass forms a logged sample again from the sample as read: the same operation, the same bits.
#include <hip/hip_runtime.h>

#include "dsp_kernels.h"
#include "dsp_lane_tiles.h"
#include "dsp_launch.h"
#include "dsp_wave.h"

namespace {

using namespace dsp_tailfit;
static_assert(POLY_MAX == DSP_POLY_MAX, "one limit");

__device__ __forceinline__ float log_of(float x) { return (float)log((double)x); }
__device__ __forceinline__ double log_of(double x) { return log(x); }
__device__ __forceinline__ float sqrt_of(float x) { return (float)sqrt((double)x); }  // (a float64 root rounds to the float32 root)
__device__ __forceinline__ double sqrt_of(double x) { return sqrt(x); }

template <typename T, typename InT, bool VEC>
__global__ __launch_bounds__(64) void dsp_tailfit_kernel(TailfitArgs A, int64_t n_wf, int* err) {
    __shared__ T tile[ROWS * PITCH];
    __shared__ double pw[TS * POLY_MAX];  // pw[u * POLY_MAX + j] = float64((s0 + u)**j) of the tile at s0
    (void)err;  // (nothing here is an error of the reference's)
    const int lane = lane_id();
    const int64_t r0 = (int64_t)blockIdx.x * ROWS, row = r0 + lane;
    const bool live = row < n_wf;
    const int rows_here = (int)(n_wf - r0 < ROWS ? n_wf - r0 : ROWS);
    const InT* __restrict__ g = (const InT*)A.wf + A.wf_offset;
    const int n = A.len, m = A.m;
    const bool do_log = A.log != 0, fit = A.fit != 0, store_log = A.out != nullptr, resid_log = A.resid_log != 0;
    const int resid = A.resid;
    const T nanv = quiet_nan<T>();
    T* outp = (T*)A.out;
    const bool wide_out = A.out_vec != 0 && rows_here == ROWS;
    // a bl_subtract of the rows that nothing else reads is done here, as they are read: one subtraction in the loop's type (bl_subtract.py:45)
    const bool sub = A.sub_mode != 0;
    const T bl = sub && live ? (A.sub ? ((const T*)A.sub)[row * A.sub_stride] : (T)A.sub_const) : (T)0;

    // ---- a lane's state
    bool in_nan = false, nonpos = false, w_nan = false, p_nan = false;
    double arr[POLY_MAX], p[POLY_MAX];  // the moments; the coefficients of the residuals, as stored
#pragma unroll
    for (int j = 0; j < POLY_MAX; ++j) arr[j] = 0.0, p[j] = 0.0;
    T mean = (T)0, rms = (T)0;
    if (resid != 0 && !fit && live) {
        const T* pars = (const T*)A.pars + A.pars_offset + row * A.pars_stride;
#pragma unroll
        for (int j = 0; j < POLY_MAX; ++j) {
            if (j >= m) break;
            const T c = pars[j];
            p_nan |= c != c;
            p[j] = (double)c;
        }
    }

    // lane u forms the powers of sample s0 + u: the integer product (where it would wrap, the planner has refused), converted once
    auto powers_of_tile = [&](int s0) {
        const unsigned long long i = (unsigned long long)(s0 + lane);
        unsigned long long q = 1;
#pragma unroll
        for (int j = 0; j < POLY_MAX; ++j) {
            if (j >= m) break;
            pw[lane * POLY_MAX + j] = (double)(long long)q;
            q *= i;
        }
        wave_sync();
    };
    // one sample of poly_fit.py:98-105 / :132-138
    auto residual_step = [&](T w, int u, int i) {
        double temp = 0.0;
#pragma unroll
        for (int j = 0; j < POLY_MAX; ++j) {
            if (j >= m) break;
            temp = temp + p[j] * pw[u * POLY_MAX + j];
        }
        const double r = resid == 2 ? (double)w - exp(temp) : (double)w - temp;
        mean = (T)((double)mean + r / (double)(i + 1));
        rms = (T)((double)rms + r * r);
        w_nan |= w != w;
    };

    LaneTiles<T, InT, VEC> rows(tile, g, A.wf_stride, r0, rows_here, n, lane);

    // ---- pass 1: the logarithm, the moments -- or, with coefficients from memory, the residuals
    rows.run([&](int s0, int w) {
        if (fit || resid != 0) powers_of_tile(s0);
        if (live) {
            T* mine = tile + lane * PITCH;
#pragma unroll 4
            for (int u = 0; u < w; ++u) {
                const T x = sub ? mine[u] - bl : mine[u];
                in_nan |= x != x;
                T v = x;
                if (do_log) {
                    nonpos |= x <= (T)0;
                    v = log_of(x);
                    if (store_log) mine[u] = v;
                }
                if (fit) {
                    const double vd = (double)v;
#pragma unroll
                    for (int j = 0; j < POLY_MAX; ++j) {
                        if (j >= m) break;
                        arr[j] = arr[j] + vd * pw[u * POLY_MAX + j];
                    }
                } else if (resid != 0) {
                    residual_step(v, u, s0 + u);
                }
            }
        }
        if (do_log && store_log) {
            wave_sync();
            store_lane_tile(tile, outp, A.out_stride, r0, rows_here, s0, w, lane, wide_out);
        }
    });

    // ---- behind the last tile: a bad row's logarithms are written over (log_check.py:40-46)
    const bool bad = in_nan || (do_log && nonpos);
    if (do_log && store_log) overwrite_nan_rows(__ballot(live && bad), outp, A.out_stride, r0, rows_here, n, lane);

    // ---- the coefficients: inv @ arr in registers, rounded once (poly_fit.py:32); a row with a NaN gives NaNs
    if (fit) {
        T* pars_out = A.pars_out && live ? (T*)A.pars_out + row * A.pars_out_stride : nullptr;
#pragma unroll
        for (int k = 0; k < POLY_MAX; ++k) {
            if (k >= m) break;
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < POLY_MAX; ++j) {
                if (j >= m) break;
                acc = acc + A.inv[k * m + j] * arr[j];
            }
            const T c = bad ? nanv : (T)acc;
            if (pars_out) pars_out[k] = c;
            p[k] = (double)c;
            p_nan |= c != c;
        }
    }

    // ---- pass 2: the residuals of the same rows, restaged, against the fitted coefficients
    if (fit && resid != 0) {
        rows.run([&](int s0, int w) {
            powers_of_tile(s0);
            if (live) {
                const T* mine = tile + lane * PITCH;
#pragma unroll 4
                for (int u = 0; u < w; ++u) {
                    const T x = sub ? mine[u] - bl : mine[u];
                    residual_step(resid_log ? log_of(x) : x, u, s0 + u);
                }
            }
        });
    }

    if (resid != 0 && live) {
        // poly_fit.py:107-108 / :140-141: rms /= n - 1 (n = 1: by zero, as IEEE has it), then the root; :92-93: a NaN in the row or among the
        // coefficients leaves the NaNs both were set to
        T root = sqrt_of((T)((double)rms / (double)(n - 1)));
        if (w_nan || p_nan) mean = root = nanv;
        ((T*)A.mean_out)[row * A.mean_stride] = mean;
        ((T*)A.rms_out)[row * A.rms_stride] = root;
    }
}

template <typename T, typename InT>
void launch_tailfit(const TailfitArgs* A, int64_t n_wf, int vec, int* err, hipStream_t stream) {
    const dim3 grid((unsigned)tiles(n_wf)), block(64);
    if (vec)
        hipLaunchKernelGGL((dsp_tailfit_kernel<T, InT, true>), grid, block, 0, stream, *A, n_wf, err);
    else
        hipLaunchKernelGGL((dsp_tailfit_kernel<T, InT, false>), grid, block, 0, stream, *A, n_wf, err);
}

}  // namespace

extern "C" int dsp_internal_launch_tailfit(const TailfitArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream) {
    if (n_wf <= 0) return 0;
    // (the planner's bounds and shapes: what runs, what it reads and where its results go)
    const bool coeffs = A->fit || A->resid;
    if (A->len < 1 || (!A->log && !coeffs) || (coeffs && (A->m < 1 || A->m > DSP_POLY_MAX)) || (A->fit && !A->inv) || (A->resid && !A->fit && !A->pars) ||
        (A->resid && (A->resid > 2 || !A->mean_out || !A->rms_out)) || (A->resid_log && !A->log) || (A->log && !A->fit && !A->out) || (A->out && !A->log) ||
        (A->fit && !A->resid && !A->pars_out) || (A->pars_out && !A->fit) || (A->log && A->resid && !A->fit))
        return (int)hipErrorInvalidValue;
    switch (dtype) {
        case DSP_F32: launch_tailfit<float, float>(A, n_wf, vec, err, stream); break;
        case DSP_I16: launch_tailfit<float, int16_t>(A, n_wf, vec, err, stream); break;
        case DSP_U16: launch_tailfit<float, uint16_t>(A, n_wf, vec, err, stream); break;
        default: launch_tailfit<double, double>(A, n_wf, vec, err, stream); break;
    }
    return (int)hipGetLastError();
}
