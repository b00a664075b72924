// dsp_pileup.hip -- the pile-up finder of the Ge recipes, one waveform per LANE:
//   rc_cr2 (processors/rc_cr2.py:12-94): a third-order recursion with a triple pole whose float64 state rounds at every written operation,
//   bi_level_zero_crossing_time_points (processors/time_point_thresh.py:404-532): a serial state machine on comparisons only,
// apart or in one launch, where the walk reads the filtered row as it is stored.
//
// Neither lets a row's samples be shared out among lanes without changing bits (the recursion) or the order of its decisions (the walk), so
// -- as in dsp_fit.hip and dsp_current.hip -- the 64 lanes of a wavefront run 64 rows' chains: the same operations per row, 64 independent
// chains per instruction.  Rows pass through LDS in tiles of 64 rows x 64 samples (dsp_kernels.h, dsp_pileup): written along the rows, 16
// bytes a lane where the rows are whole vectors (one tile ahead, in registers), read along the columns with a pitch of 65; a lane writes its
// filtered samples over the ones it has read, and the tile goes back to memory along the rows.
//
// A bl_subtract ahead of either (a constant or a per-event baseline) is one subtraction in the loop's type as a sample is read.
// rc_cr2: the coefficients 3a, 3(a a), a(a a) come from the host in float64 (the device's exp is not libm's); the sum runs in the written
// order, 3a w2 - 3(a a) w1 + a(a a) w0 + x[i] - 2 x[i-1] + x[i-2], one rounding at the store (-ffp-contract=off: no fused multiply-add).
// A NaN among the samples of a row is known only when the lane gets there: what the row has stored by then is written over with NaNs behind
// the last tile, and likewise the list entries of the walk.
// The walk keeps the reference's state as it is: the two "is above / is below" variables hold the sample index and are tested for truth, so
// a threshold crossing at sample 0 counts as not set; the count goes on past the lists' length; candidates start at 0.
#include <hip/hip_runtime.h>

#include "dsp_kernels.h"
#include "dsp_launch.h"
#include "dsp_wave.h"

namespace {

using namespace dsp_pileup;

__device__ __forceinline__ void pileup_report(int* err, int code, int64_t row) {
    if (atomicCAS(&err[0], 0, code) == 0) {
        err[1] = (int)(row & 0xffffffffll);
        err[2] = (int)(row >> 32);
    }
}

// VEC: rows start on 16-byte boundaries, lie whole vectors apart and hold whole vectors (the planner's and the call's word)
template <typename T, typename InT, bool VEC>
__global__ __launch_bounds__(64) void dsp_pileup_kernel(PileupArgs A, int64_t n_wf, int* err) {
    __shared__ T tile[ROWS * PITCH];
    const int lane = lane_id();
    const int64_t r0 = (int64_t)blockIdx.x * ROWS, row = r0 + lane;
    const bool live = row < n_wf;
    const int rows_here = (int)(n_wf - r0 < ROWS ? n_wf - r0 : ROWS);
    const InT* __restrict__ g = (const InT*)A.wf + A.wf_offset;
    const int n = A.len, m = A.m;
    const bool filter = A.filter != 0, walk = A.walk != 0, store_row = A.out != nullptr;
    const T nanv = quiet_nan<T>();
    T* outp = (T*)A.out;
    // a bl_subtract of the rows that nothing else reads is done here, as they are read: one subtraction in the loop's type (bl_subtract.py:45);
    // a NaN baseline makes every sample NaN, and the row a NaN row like any other
    const bool sub = A.sub_mode != 0;
    const T bl = sub && live ? (A.sub ? ((const T*)A.sub)[row * A.sub_stride] : (T)A.sub_const) : (T)0;

    // ---- the walk's operands and the reference's checks on them, in its order (time_point_thresh.py:471-488); what they find is reported
    // behind the last tile, when "a NaN in the row" -- the first of them -- is known
    auto par = [&](int k) -> T { return A.par[k] ? ((const T*)A.par[k])[row * A.par_stride[k]] : (T)A.par_const[k]; };
    T pos = (T)0, neg = (T)0, gate_f = (T)0, ts_f = (T)0;
    if (walk && live) {
        pos = par(0);
        neg = par(1);
        gate_f = par(2);
        ts_f = par(3);
    }
    const bool par_nan = pos != pos || neg != neg || ts_f != ts_f || !(__builtin_fabs((double)gate_f) <= 1.7976931348623157e308);
    int pending = 0;  // a DSP_E_* of t_start
    if (walk && live && !par_nan) {
        if (floor(ts_f) != ts_f) pending = DSP_E_TPT_START_INT;
        else if (ts_f < (T)0 || ts_f >= (T)n) pending = DSP_E_TPT_RANGE;
    }
    const bool walking = walk && live && !par_nan && pending == 0;
    const int ts = walking ? (int)ts_f : 0;
    // int(gate_time_in): towards zero; beyond the integers a row can be apart, the nearest of them decides the same way
    const int gate = gate_f >= (T)1073741824 ? 1073741824 : (gate_f <= (T)-1073741824 ? -1073741824 : (int)gate_f);
    T* pol_out = (T*)A.list[0] + row * A.list_stride[0];
    T* time_out = (T*)A.list[1] + row * A.list_stride[1];

    // ---- a lane's state
    const double c1 = A.c1, c2 = A.c2, c3 = A.c3;
    double w0 = 0.0, w1 = 0.0, w2 = 0.0, x1 = 0.0, x2 = 0.0;  // the filter's outputs and inputs before this sample, float64
    bool in_nan = false, out_nan = false;
    int above = 0, below = 0, pos_cand = 0, neg_cand = 0;  // (an index, 0: not set -- the reference tests them for truth)
    bool crossed = false;
    unsigned count = 0;
    T prev = (T)0;  // the walk's w_in[i] while the lane is at sample i + 1

    auto found = [&](int cand, T polarity) {
        if (count < (unsigned)m) {
            time_out[count] = (T)cand;
            pol_out[count] = polarity;
        }
        ++count;
    };
    // one step of time_point_thresh.py:494-532 at sample i: the four tests in the reference's order
    auto step = [&](T wi, T wn, int i) {
        if (below && wi <= (T)0 && (T)0 < wn) {
            crossed = true;
            neg_cand = i;
        }
        if (wi <= pos && pos < wn) {
            if (crossed && below) {
                if (i - below < gate) found(neg_cand, (T)0);
                else above = i;
                below = 0;
                crossed = false;
            } else {
                above = i;
            }
        }
        if (above && wi >= (T)0 && (T)0 > wn) {
            crossed = true;
            pos_cand = i;
        }
        if (wi >= neg && neg > wn) {
            if (crossed && above) {
                if (i - above < gate) found(pos_cand, (T)1);
                else below = i;
                above = 0;
                crossed = false;
            } else {
                below = i;
            }
        }
    };

    // ---- the tiles.  Whole tiles of whole blocks are fetched with 16-byte loads -- V samples of a row per lane, V rows per instruction --
    // one tile ahead (dsp_fit.hip's loader); the last rows of a batch, the last samples of a row and rows that are not whole vectors take the
    // element-wise path.
    constexpr int V = 16 / (int)sizeof(InT), NV = TS / V;  // samples per load, loads per lane and tile
    typedef InT vec_t __attribute__((ext_vector_type(V)));
    const bool wide = VEC && rows_here == ROWS;
    vec_t pf[NV];
    const int pr = lane / (TS / V), pc = (lane % (TS / V)) * V;  // row within a group of V rows, first sample of this lane's piece
    auto fetch = [&](int s0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) pf[q] = *(const vec_t*)(g + (r0 + q * V + pr) * A.wf_stride + s0 + pc);
    };
    auto commit = [&]() {
#pragma unroll
        for (int q = 0; q < NV; ++q)
#pragma unroll
            for (int e = 0; e < V; ++e) tile[(q * V + pr) * PITCH + pc + e] = (T)pf[q][e];
    };
    constexpr int VO = 16 / (int)sizeof(T), NVO = TS / VO;  // the same for the stores of the filtered row
    typedef T ovec_t __attribute__((ext_vector_type(VO)));
    const bool wide_out = A.out_vec != 0 && rows_here == ROWS;
    const int por = lane / (TS / VO), poc = (lane % (TS / VO)) * VO;

    if (wide && n >= TS) fetch(0);
    for (int s0 = 0; s0 < n; s0 += TS) {
        const int w = n - s0 < TS ? n - s0 : TS;
        if (wide && w == TS) {
            commit();
            if (s0 + 2 * TS <= n) fetch(s0 + TS);
        } else {
#pragma unroll 8
            for (int r = 0; r < rows_here; ++r) tile[r * PITCH + lane] = lane < w ? (T)g[(r0 + r) * A.wf_stride + s0 + lane] : (T)0;
        }
        wave_sync();
        if (live) {
            T* mine = tile + lane * PITCH;
#pragma unroll 8
            for (int u = 0; u < w; ++u) {
                const int j = s0 + u;  // (uniform)
                const T x = sub ? mine[u] - bl : mine[u];
                in_nan |= x != x;
                T v = x;
                if (filter) {
                    const double xd = (double)x;
                    double s;
                    if (j < 3) {  // rc_cr2.py:56-64
                        s = xd;
                    } else {  // rc_cr2.py:77-86, the terms in the written order
                        s = c1 * w2;
                        s = s - c2 * w1;
                        s = s + c3 * w0;
                        s = s + xd;
                        s = s + -2.0 * x1;
                        s = s + x2;
                    }
                    v = j < 3 ? x : (T)s;
                    w0 = w1;
                    w1 = w2;
                    w2 = s;
                    x2 = x1;
                    x1 = xd;
                    out_nan |= v != v;
                    if (store_row) mine[u] = v;
                }
                if (walking && j > ts) step(prev, v, j - 1);  // i = j - 1 in [t_start, n - 2]
                prev = v;
            }
        }
        if (store_row) {
            wave_sync();
            if (wide_out && w == TS) {
#pragma unroll
                for (int q = 0; q < NVO; ++q) {
                    ovec_t o;
#pragma unroll
                    for (int e = 0; e < VO; ++e) o[e] = tile[(q * VO + por) * PITCH + poc + e];
                    *(ovec_t*)(outp + (r0 + q * VO + por) * A.out_stride + s0 + poc) = o;
                }
            } else {
#pragma unroll 8
                for (int r = 0; r < rows_here; ++r)
                    if (lane < w) outp[(r0 + r) * A.out_stride + s0 + lane] = tile[r * PITCH + lane];
            }
        }
        wave_sync();
    }

    // ---- behind the last tile.  A row with a NaN, and every row for a NaN t_tau, is a NaN row (rc_cr2.py:46-49): what it has stored is
    // written over, once the stores before are done.  A NaN of the filter's own making is the reference's DSPFatal.
    const bool row_nan = in_nan || (filter && A.tau_nan != 0);
    if (filter && store_row) {
        const unsigned long long nan_rows = __ballot(live && row_nan);
        if (nan_rows) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            for (int r = 0; r < rows_here; ++r)
                if ((nan_rows >> r) & 1ull)
                    for (int k = lane; k < n; k += 64) outp[(r0 + r) * A.out_stride + k] = nanv;
        }
    }
    if (!live) return;
    const bool made_nan = filter && out_nan && !row_nan;
    if (made_nan) pileup_report(err, DSP_E_RC_CR2_NAN, row);
    if (walk) {
        // the walk of a NaN row, or with a NaN operand, returns before it counts (time_point_thresh.py:471-477): NaN lists, and the count 0
        const bool none = row_nan || made_nan || par_nan || pending != 0;
        if (none && count > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int first = none ? 0 : (int)(count < (unsigned)m ? count : (unsigned)m);
        for (int k = first; k < m; ++k) {
            time_out[k] = nanv;
            pol_out[k] = nanv;
        }
        A.n_out[row * A.n_stride] = none ? 0u : count;
        if (pending != 0 && !row_nan && !made_nan) pileup_report(err, pending, row);
    }
}

template <typename T, typename InT>
void launch_pileup(const PileupArgs* A, int64_t n_wf, int vec, int* err, hipStream_t stream) {
    const dim3 grid((unsigned)tiles(n_wf)), block(64);
    if (vec)
        hipLaunchKernelGGL((dsp_pileup_kernel<T, InT, true>), grid, block, 0, stream, *A, n_wf, err);
    else
        hipLaunchKernelGGL((dsp_pileup_kernel<T, InT, false>), grid, block, 0, stream, *A, n_wf, err);
}

}  // namespace

extern "C" int dsp_internal_launch_pileup(const PileupArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream) {
    if (n_wf <= 0) return 0;
    // (the planner's bounds: the recursion reads three samples back; a list entry per crossing up to m)
    if (A->len < 1 || (A->filter && A->len < MIN_FILTER_LEN) || (!A->filter && !A->walk) || (A->walk && (A->m < 1 || !A->list[0] || !A->list[1] || !A->n_out)) ||
        (!A->walk && !A->out))
        return (int)hipErrorInvalidValue;
    switch (dtype) {
        case DSP_F32: launch_pileup<float, float>(A, n_wf, vec, err, stream); break;
        case DSP_I16: launch_pileup<float, int16_t>(A, n_wf, vec, err, stream); break;
        case DSP_U16: launch_pileup<float, uint16_t>(A, n_wf, vec, err, stream); break;
        default: launch_pileup<double, double>(A, n_wf, vec, err, stream); break;
    }
    return (int)hipGetLastError();
}
