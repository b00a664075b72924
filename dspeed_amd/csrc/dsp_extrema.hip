// dsp_extrema.hip -- get_multi_local_extrema (processors/get_multi_local_extrema.py:12-306): the lists of local maxima and minima of a row,
// found by a hysteresis state machine over its samples.  The only processor here whose result is a list.
//
// A wavefront per row, four to a workgroup, the row streamed through registers as dsp_row_stream.h lays it out (16 bytes per lane and load,
// four loads in flight, non-temporal; a sample per lane where start, stride or length are not whole 16-byte vectors).  The machine looks
// sequential -- "the sample is more than delta below the running maximum: tag that maximum, look for a minimum from here" -- but between
// two transitions it is a prefix maximum (or minimum) and a comparison per sample.  One sweep, in sweep order (forward: sample p;
// backward: sample n - 1 - p), reference lines 135-200:
//   state: find_max, the running extreme (value, position; first occurrence, as the strict comparisons make it), two counters.  Only one
//   running extreme matters at a time: the reference tracks the other as well but overwrites it at every transition.
//   a group of 64 N consecutive samples, lane l holding N of them (N = 1, or the samples of a 16-byte vector):
//     1. inclusive prefix maximum with its position over the group, carried in from the running extreme: sequential over a lane's own
//        samples, one scan of the lanes' totals across the wavefront, the lane below's result carried into each lane
//     2. every sample's trigger against its prefix value p:  w < p - delta  (one rounding in the loop's type, as w_in[imax] - a_delta_max_in
//        has)  and  count < m  and  p > a_abs_max
//     3. ballot.  None: the group's total is the running extreme, next group.  Some: the first one, sample k -- tag the prefix extreme as of
//        k, flip the state, the running extreme is sample k itself, and the rest of the group, from k + 1 on, is looked at again.
//   The minimum state is the same machine on the negated samples:  w > w[imin] + d  is  -w < (-w[imin]) - d  with the same rounding, and
//   w[imin] < a  is  -w[imin] > -a.
// About one step per group and one per extremum found.  tests/test_extrema_cases_cpu.py holds this formulation in NumPy for every N the
// kernels are built with and compares it with the reference's body.
//
// Outputs (reference lines 98-124, 202-215, 288-303): indices in the loop's float type in the order found, NaN-padded to m; counts as
// uint32; a NaN anywhere in the row or a NaN delta: NaN arrays and counts 0 -- known only when the row has been read, so indices written
// on the way are overwritten by the same wavefront at the end.  search_direction 3 runs both sweeps with the tags in registers (tag c in
// lane c: m <= 64) and writes the first m of their sorted, de-duplicated union.
#include <hip/hip_runtime.h>

#include "dsp_launch.h"
#include "dsp_row_stream.h"
#include "dsp_wave.h"

namespace {

// lanes without a source keep their own value: combining a value with itself changes nothing in a running maximum
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_self(int v) {
    return __builtin_amdgcn_update_dpp(v, v, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_self(float v) {
    return __int_as_float(dpp_self<CTRL, ROW_MASK>(__float_as_int(v)));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_self(double v) {
    const int lo = dpp_self<CTRL, ROW_MASK>(__double2loint(v));
    const int hi = dpp_self<CTRL, ROW_MASK>(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// one step of the inclusive scan: (ov, op) comes from lanes below, so it is the earlier one and stays on a tie
template <int CTRL, int ROW_MASK, typename T>
__device__ __forceinline__ void scan_step(T& v, int& p) {
    const T ov = dpp_self<CTRL, ROW_MASK>(v);
    const int op = dpp_self<CTRL, ROW_MASK>(p);
    const bool later = v > ov;
    v = later ? v : ov;
    p = later ? p : op;
}
template <typename T>
__device__ __forceinline__ void wave_scan_max_first(T& v, int& p) {
    scan_step<DPP_ROW_SHR1, 0xf>(v, p);
    scan_step<DPP_ROW_SHR2, 0xf>(v, p);
    scan_step<DPP_ROW_SHR4, 0xf>(v, p);
    scan_step<DPP_ROW_SHR8, 0xf>(v, p);
    scan_step<DPP_ROW_BCAST15, 0xa>(v, p);
    scan_step<DPP_ROW_BCAST31, 0xc>(v, p);
}
// the lane below's value; lane 0 gets `first`
__device__ __forceinline__ int below(int v, int first) { return __builtin_amdgcn_update_dpp(first, v, DPP_WAVE_SHR1, 0xf, 0xf, false); }
__device__ __forceinline__ float below(float v, float first) { return __int_as_float(below(__float_as_int(v), __float_as_int(first))); }
__device__ __forceinline__ double below(double v, double first) {
    const int lo = below(__double2loint(v), __double2loint(first));
    const int hi = below(__double2hiint(v), __double2hiint(first));
    return __hiloint2double(hi, lo);
}

template <typename T>
struct Sweep {
    bool mx;      // looking for a maximum
    T rv;         // the running extreme in the state's sign (negated while a minimum is looked for) ...
    int rp;       // ... and its position in sweep order
    int cmax, cmin;  // maxima, minima tagged
    bool nan;        // a NaN among the lane's samples
    int tmax, tmin;  // keep: tag c of each list in lane c (as a sample index)
};

// One group: the 64 N samples at sweep positions base .. base + 64 N - 1, lane l holding x[j] = position base + l N + j (positions >= n are
// dead).  `keep`: the tags stay in registers (search_direction 3), else lane 0 writes each to its place as it is found.
template <typename T, int N>
__device__ __forceinline__ void extrema_group(Sweep<T>& S, const T (&x)[N], int base, int n, int m, bool back, T dmax, T dmin, T amax, T amin,
                                              bool keep, T* out_max, T* out_min, int lane) {
    const T ninf = -__builtin_inff();
    const int p0 = base + lane * N;
    int q = -1;  // positions up to q have been dealt with (uniform)
#pragma unroll
    for (int j = 0; j < N; ++j) S.nan |= p0 + j < n && x[j] != x[j];
    for (;;) {
        // 1. the lane's own prefix, then the lanes' totals across the wavefront with the running extreme carried in at lane 0
        T y[N], lv[N];
        int lp[N];
        bool alive[N];
        T cv = ninf;
        int cp = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            y[j] = S.mx ? x[j] : -x[j];
            alive[j] = p0 + j > q && p0 + j < n;
            const bool t = alive[j] && y[j] > cv;
            cv = t ? y[j] : cv;
            cp = t ? p0 + j : cp;
            lv[j] = cv;
            lp[j] = cp;
        }
        T tv = cv;
        int tp = cp;
        {
            const bool own = lane != 0 || tv > S.rv;
            tv = own ? tv : S.rv;
            tp = own ? tp : S.rp;
        }
        wave_scan_max_first(tv, tp);
        const T ev = below(tv, S.rv);
        const int ep = below(tp, S.rp);
        // 2. the triggers, last sample first so that the lane's first one is what it holds
        const T d = S.mx ? dmax : dmin, a = S.mx ? amax : -amin;
        const bool room = (S.mx ? S.cmax : S.cmin) < m;
        bool hit = false;
        int hit_tag = 0, hit_j = 0;
        T hit_y = (T)0;
#pragma unroll
        for (int j = N - 1; j >= 0; --j) {
            const bool later = lv[j] > ev;
            const T pv = later ? lv[j] : ev;
            const int pp = later ? lp[j] : ep;
            const bool trig = alive[j] && room && y[j] < pv - d && pv > a;
            hit |= trig;
            hit_tag = trig ? pp : hit_tag;
            hit_j = trig ? j : hit_j;
            hit_y = trig ? y[j] : hit_y;
        }
        // 3. nobody: the group's total runs on; somebody: the first one
        const unsigned long long mask = __ballot(hit);
        if (!mask) {
            S.rv = readlane(tv, 63);
            S.rp = readlane(tp, 63);
            return;
        }
        const int k = __builtin_ctzll(mask);
        const int tagged = readlane(hit_tag, k), kj = readlane(hit_j, k);
        const T ky = readlane(hit_y, k);
        const int index = back ? n - 1 - tagged : tagged;
        if (S.mx) {
            if (keep) S.tmax = lane == S.cmax ? index : S.tmax;
            else if (lane == 0) out_max[S.cmax] = (T)index;
            ++S.cmax;
        } else {
            if (keep) S.tmin = lane == S.cmin ? index : S.tmin;
            else if (lane == 0) out_min[S.cmin] = (T)index;
            ++S.cmin;
        }
        q = base + k * N + kj;
        S.rv = -ky;
        S.rp = q;
        S.mx = !S.mx;
    }
}

template <typename T, typename IN, int N>
__device__ __forceinline__ void extrema_sweep(Sweep<T>& S, const IN* w, int n, int m, bool back, T dmax, T dmin, T amax, T amin, bool keep, T* out_max,
                                              T* out_min, int lane) {
    typedef typename RowVec<IN>::vec vec;
    S.mx = true;
    S.rv = (T)w[back ? n - 1 : 0];
    S.rp = 0;
    S.cmax = S.cmin = 0;
    const int per_group = 64 * N, n_groups = (n + per_group - 1) / per_group;
    for (int g0 = 0; g0 < n_groups; g0 += 4) {
        T x[4][N];
        if constexpr (N > 1) {
            // (whole vectors: n is a multiple of N, a vector that starts inside the row lies inside it; backward, the vector that holds
            // sweep positions p0 .. p0 + N - 1 starts at sample n - p0 - N and is read last element first)
            const vec* wv = (const vec*)w;
            vec v[4] = {};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int p0 = (g0 + k) * per_group + lane * N;
                if (p0 < n) v[k] = __builtin_nontemporal_load(wv + (back ? (n - p0 - N) / N : p0 / N));
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < N; ++j) x[k][j] = back ? (T)v[k][N - 1 - j] : (T)v[k][j];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int p0 = (g0 + k) * 64 + lane;
                x[k][0] = p0 < n ? (T)w[back ? n - 1 - p0 : p0] : (T)0;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((g0 + k) * per_group < n)  // (uniform)
                extrema_group<T, N>(S, x[k], (g0 + k) * per_group, n, m, back, dmax, dmin, amax, amin, keep, out_max, out_min, lane);
    }
}

// search_direction 3: the forward tags (ascending, tag c in lane c, nf of them) and the backward ones (descending, nb) of one kind; writes the
// first m of the sorted union without duplicates and returns min(m, its size)
template <typename T>
__device__ __forceinline__ int write_union(int f, int nf, int b, int nb, int m, T* out, int lane) {
    bool dup = false;  // the lane's backward tag is also a forward one
    int f_below_b = 0;
    for (int s = 0; s < nf; ++s) {
        const int fs = readlane(f, s);
        dup |= fs == b;
        f_below_b += fs < b ? 1 : 0;
    }
    dup = dup && lane < nb;
    const unsigned long long dups = __ballot(dup);
    int b_below_f = 0, b_below_b = 0;  // backward tags that are no duplicates, below the lane's forward / backward tag
    for (int s = 0; s < nb; ++s) {
        const int bs = readlane(b, s);
        const bool counts = !((dups >> s) & 1ull);
        b_below_f += counts && bs < f ? 1 : 0;
        b_below_b += counts && bs < b ? 1 : 0;
    }
    const int n_dup = __builtin_popcountll(dups);
    const int rank_f = lane + b_below_f, rank_b = f_below_b + b_below_b;
    if (lane < nf && rank_f < m) out[rank_f] = (T)f;
    if (lane < nb && !dup && rank_b < m) out[rank_b] = (T)b;
    const int size = nf + nb - n_dup;
    return size < m ? size : m;
}

template <typename T, typename IN, int N>
__global__ void __launch_bounds__(256) dsp_extrema_kernel(ExtremaArgs A, int64_t n_wf, int* err) {
    const int lane = lane_id();
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= n_wf) return;  // (whole wavefronts: no barrier in this kernel)
    const IN* w = (const IN*)A.wf + row * A.wf_stride + A.wf_offset;
    const int n = A.len, m = A.m;
    T par[4];  // a_delta_max, a_delta_min, a_abs_max, a_abs_min
#pragma unroll
    for (int k = 0; k < 4; ++k) par[k] = A.par[k] ? ((const T*)A.par[k])[row * A.par_stride[k]] : (T)A.par_const[k];
    T* out_max = (T*)A.vt_out[0] + row * A.vt_stride[0];
    T* out_min = (T*)A.vt_out[1] + row * A.vt_stride[1];
    Sweep<T> S;
    S.nan = false;
    S.tmax = S.tmin = 0;
    int count[2];
    if (A.direction == 3) {
        extrema_sweep<T, IN, N>(S, w, n, m, false, par[0], par[1], par[2], par[3], true, out_max, out_min, lane);
        const int f_max = S.tmax, f_min = S.tmin, nf_max = S.cmax, nf_min = S.cmin;
        extrema_sweep<T, IN, N>(S, w, n, m, true, par[0], par[1], par[2], par[3], true, out_max, out_min, lane);
        count[0] = write_union<T>(f_max, nf_max, S.tmax, S.cmax, m, out_max, lane);
        count[1] = write_union<T>(f_min, nf_min, S.tmin, S.cmin, m, out_min, lane);
    } else {
        extrema_sweep<T, IN, N>(S, w, n, m, A.direction == 1, par[0], par[1], par[2], par[3], false, out_max, out_min, lane);
        count[0] = S.cmax;
        count[1] = S.cmin;
    }
    // the NaN rule, the padding, the counts (reference lines 98-124)
    const bool all_nan = wave_any(S.nan) || par[0] != par[0] || par[1] != par[1];
    if (all_nan) count[0] = count[1] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // the tags written above are on their way before anything here overwrites them
    const T nanv = quiet_nan<T>();
    for (int j = count[0] + lane; j < m; j += 64) out_max[j] = nanv;
    for (int j = count[1] + lane; j < m; j += 64) out_min[j] = nanv;
    if (lane == 0) {
        A.n_out[0][row * A.n_stride[0]] = (uint32_t)count[0];
        A.n_out[1][row * A.n_stride[1]] = (uint32_t)count[1];
        // a delta per event: "Delta must be positive" (reference lines 130-131) for the rows that got past the NaN rule
        if (!all_nan && (!(par[0] >= (T)0) || !(par[1] >= (T)0)) && atomicCAS(&err[0], 0, DSP_E_EXTREMA_DELTA) == 0) {
            err[1] = (int)(row & 0xffffffffll);
            err[2] = (int)(row >> 32);
        }
    }
}

template <typename T, typename IN>
void launch_extrema(const ExtremaArgs* A, int64_t n_wf, int vec, int* err, hipStream_t stream) {
    const unsigned blocks = row_blocks(n_wf);
    if (vec)
        hipLaunchKernelGGL((dsp_extrema_kernel<T, IN, RowVec<IN>::N>), dim3(blocks), dim3(256), 0, stream, *A, n_wf, err);
    else
        hipLaunchKernelGGL((dsp_extrema_kernel<T, IN, 1>), dim3(blocks), dim3(256), 0, stream, *A, n_wf, err);
}

}  // namespace

extern "C" int dsp_internal_launch_extrema(const ExtremaArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream) {
    if (n_wf <= 0) return 0;
    switch (dtype) {
        case DSP_F32: launch_extrema<float, float>(A, n_wf, vec, err, stream); break;
        case DSP_I16: launch_extrema<float, int16_t>(A, n_wf, vec, err, stream); break;
        case DSP_U16: launch_extrema<float, uint16_t>(A, n_wf, vec, err, stream); break;
        case DSP_F64: launch_extrema<double, double>(A, n_wf, vec, err, stream); break;
        case DSP_I32: launch_extrema<double, int32_t>(A, n_wf, vec, err, stream); break;
        default: launch_extrema<double, uint32_t>(A, n_wf, vec, err, stream); break;
    }
    return (int)hipGetLastError();
}
