// dsp_interp.hip -- interpolating_upsampler (processors/upsampler.py:52-216): every row of n samples resampled to m outputs by one of seven
// rules -- 'i' zero-stuffing, 'n' nearest, 'f' floor, 'c' ceiling, 'l' linear, 'h' Hermite cubic, 's' natural cubic spline.  A row that
// holds a NaN comes out as NaNs.  m / n is a float64 and need not be an integer, or above 1.
//
// The reference walks the input samples and fills intervals of outputs; this kernel keeps the row in LDS and walks the outputs, every lane
// V consecutive ones, so that the stores -- what bounds a kernel whose output is longer than its input -- are coalesced.  The index rules
// (which input segment an output belongs to, in the reference's own float64 bound expressions) are dsp_kernels.h's, dsp_interp, shared
// with the planner and tests/interp_index.cpp.
//   geometry   rows of up to 8 KiB of LDS get a wavefront each, four to a workgroup, and need no barrier; longer ones a workgroup of 256.
//              Both are this one kernel: WIDE chooses what "everybody" means.  A wide row's wavefronts agree on "a NaN" / "an infinity"
//              through one word behind the row (16 bytes past the 64 KiB of the longest rows: dsp_internal_set_interp_lds).
//   staging    the shared loader (dsp_row_stream.h) into LDS, in the loop's type; the NaN screen happens here.
//   arithmetic numba's typing of the reference: t, the polynomial weights and the spline's sweeps are float64, differences of two samples
//              are rounded to the loop's type first, everything they meet is float64, the store rounds; cubes are x * (x * x).  One
//              rounding per written operation (the library is built with -ffp-contract=off).
//   mode 's'   two passes ahead of the evaluation, both over a lane's chunk of neighbouring samples from a warm-up of 48 (dsp_interp::WARM):
//              u[i] of the forward sweep in the reference's operation order (its coefficient is data independent, stationary from sample
//              15 on), then the second derivatives from a warm-up on the far side -- every lane first finds the value above its chunk
//              from u alone, then, behind a barrier, overwrites its chunk of u.  They live in LDS as float64 behind the row.  Chunks are
//              an odd number of samples long: lanes' 8-byte accesses a chunk apart then fall into different pairs of banks.  A row with
//              an infinite sample, which no warm-up window can see, runs the reference's two sweeps in order on one lane.
//   stores     16 bytes per lane where the output rows' start and stride are whole vectors (InterpArgs::out_vec) and the lane's outputs
//              lie inside the row whole, else a sample per lane; non-temporal: the row is not read again.  The reference's store one
//              past the end in mode 's' (w_out[len(w_out)]) is not made.
#include <hip/hip_runtime.h>

#include "dsp_kernels.h"
#include "dsp_launch.h"
#include "dsp_row_stream.h"
#include "dsp_wave.h"

namespace {

using namespace dsp_interp;

constexpr int STEP = 0;  // the modes that copy a sample or write a zero: 'i' 'n' 'f' 'c' (which one: at run time)

// output o of the row, from segment mp: MODE is STEP, 'l', 'h' or 's'
template <typename T, int MODE>
__device__ __forceinline__ T eval(const T* x, const double* w2, int n, double u, int64_t o, Map mp) {
    if (mp.kind == NONE) return quiet_nan<T>();
    const int i = mp.seg;
    if constexpr (MODE == STEP) {
        return mp.kind == ZERO ? (T)0 : x[i];
    } else if constexpr (MODE == 'l') {
        const T a = x[i], a_next = x[i < n - 1 ? i + 1 : n - 1];
        const double t = (double)o / u - (double)i;
        return (T)((double)a + t * (double)(T)(a_next - a));
    } else if constexpr (MODE == 'h') {
        const double t0 = (double)o / u - (double)i, t1 = 1.0 - t0;
        const double m0 = i == 0 ? (double)(T)(x[1] - x[0]) : (double)(T)(x[i + 1] - x[i - 1]) / 2.0;
        const double m1 = i == n - 2 ? (double)(T)(x[n - 1] - x[n - 2]) : (double)(T)(x[i + 2] - x[i]) / 2.0;
        const double t1_2 = t1 * t1, t1_3 = t1 * t1_2, t0_2 = t0 * t0, t0_3 = t0 * t0_2;
        return (T)((((-2.0 * t1_3 + 3.0 * t1_2) * (double)x[i] + (-2.0 * t0_3 + 3.0 * t0_2) * (double)x[i + 1]) - (t1_3 - t1_2) * m0) +
                   (t0_3 - t0_2) * m1);
    } else {
        const double t0 = (double)o / u - (double)i, t1 = 1.0 - t0;
        const double t1_3 = t1 * (t1 * t1), t0_3 = t0 * (t0 * t0);
        return (T)((t1 * (double)x[i] + t0 * (double)x[i + 1]) + ((t1_3 - t1) * w2[i] + (t0_3 - t0) * w2[i + 1]) / 6.0);
    }
}

// the outputs of a row: thread `tid` of G takes V consecutive ones a turn
template <typename T, int MODE, int V, int G>
__device__ __forceinline__ void write_row(T* out, const T* x, const double* w2, int n, int64_t m, int mode, int tid) {
    typedef T Vec __attribute__((ext_vector_type(V > 1 ? V : 2)));
    const double u = ratio(n, m);
    for (int64_t o0 = (int64_t)tid * V; o0 < m; o0 += (int64_t)G * V) {
        T v[V];
        int i = mode == 'i' ? 0 : locate(mode, n, u, o0);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int64_t o = o0 + j;
            if (j > 0 && mode != 'i') i = advance(mode, n, u, o, i);
            v[j] = o < m ? eval<T, MODE>(x, w2, n, u, o, map_of(mode, n, m, o, i)) : (T)0;
        }
        if constexpr (V > 1) {
            if (o0 + V <= m) {
                Vec q;
#pragma unroll
                for (int j = 0; j < V; ++j) q[j] = v[j];
                __builtin_nontemporal_store(q, (Vec*)(out + o0));
                continue;
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (o0 + j < m) __builtin_nontemporal_store(v[j], out + o0 + j);
    }
}

// N: samples per lane and load (dsp_row_stream.h); WIDE: a workgroup per row, else a wavefront; OV: 16-byte stores
template <typename T, typename IN, int N, bool WIDE, bool OV>
__global__ void __launch_bounds__(256) dsp_interp_kernel(InterpArgs A, int64_t n_wf) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int K = N > 1 ? 4 : 8;    // loads in flight
    constexpr int G = WIDE ? 256 : 64;  // threads of a row
    constexpr int NW = WIDE ? 4 : 1;    // wavefronts of a row
    constexpr int V = OV ? 16 / (int)sizeof(T) : 1;
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const int tid = WIDE ? (int)threadIdx.x : lane;
    const int64_t row = WIDE ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + wave;
    if (!WIDE && row >= n_wf) return;  // (whole wavefronts, and no barrier in this geometry; WIDE: the grid is n_wf)
    const int n = A.len, mode = A.mode;
    const int64_t m = A.out_len;
    const int rb = row_bytes(mode, n, (int)sizeof(T));
    unsigned char* mine = lds_raw + (WIDE ? 0 : wave * rb);
    T* x = (T*)mine;
    double* w2 = (double*)(mine + w2_offset(n, (int)sizeof(T)));  // (mode 's')
    int* row_flags = (int*)(lds_raw + rb);                        // (WIDE) bit 0: a NaN, bit 1: an infinity
    const IN* w = (const IN*)A.wf + row * A.wf_stride + A.wf_offset;
    auto everybody = [&]() {
        if constexpr (WIDE)
            __syncthreads();
        else
            wave_sync();
    };

    // staging
    if constexpr (WIDE) {
        if (tid == 0) *row_flags = 0;
        __syncthreads();
    }
    bool bad = false, inf = false;
    for (int g0 = (WIDE ? wave : 0) * K; g0 < row_groups<N>(n); g0 += NW * K) {
        T s[K][N];
        load_row_groups<T, IN, N, K>(s, w, n, g0, lane);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int at = in_row<N>(g0, k, 0, lane);
            if (at >= n) continue;  // (n is a multiple of N: a vector that starts inside the row lies inside it whole)
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const T v = s[k][j];
                bad |= v != v;
                inf |= !((v - v) == (T)0);
                x[at + j] = v;
            }
        }
    }
    bad = wave_any(bad);
    inf = wave_any(inf);
    if constexpr (WIDE) {
        if ((bad || inf) && lane == 0) atomicOr(row_flags, (bad ? 1 : 0) | (inf ? 2 : 0));
        __syncthreads();  // (also the barrier behind the staging)
        bad = (*row_flags & 1) != 0;
        inf = (*row_flags & 2) != 0;
    } else {
        wave_sync();
    }

    T* out = (T*)A.out + row * A.out_stride;
    if (bad) {
        const T nanv = quiet_nan<T>();
        for (int64_t o = tid; o < m; o += G) out[o] = nanv;
        return;  // (everybody of the row: `bad` is the row's)
    }

    if (mode == 's' && n >= 2) {
        constexpr double P_FIX = 0.5 * W2_FIX + 2.0;
        if (tid == 0) w2[0] = 0.0, w2[n - 1] = 0.0;  // (np.zeros: the natural ends; the back substitution leaves them 0 on a finite row)
        if (inf) {
            // the reference's two sweeps, in order, on one lane: u alternates +-inf from the sample on and the back substitution carries that down
            if (tid == 0) {
                double wc = 0.0, uu = 0.0;
                for (int i = 1; i <= n - 2; ++i) {
                    const double p = 0.5 * wc + 2.0;
                    wc = -0.5 / p;
                    const double d = ((double)x[i + 1] - 2.0 * (double)x[i]) + (double)x[i - 1];
                    uu = (3.0 * d - 0.5 * uu) / p;
                    w2[i] = uu;
                }
                double W = 0.0;
                for (int i = n - 2; i >= 0; --i) {
                    W = forward_coef(i) * W + (i >= 1 ? w2[i] : 0.0);
                    w2[i] = W;
                }
            }
            everybody();
        } else {
            const int L = ((n + G - 1) / G) | 1;  // an odd chunk: 8-byte accesses a chunk apart fall into different pairs of banks
            const int a = tid * L, b = a + L < n ? a + L : n;
            const int lo = a > 1 ? a : 1, hi = b < n - 1 ? b : n - 1;  // the chunk's part of 1 .. n - 2: [lo, hi)
            if (lo < hi) {
                const int s = lo - WARM > 1 ? lo - WARM : 1;
                double wc = forward_coef(s - 1), uu = 0.0;
                for (int i = s; i < hi; ++i) {
                    double p = P_FIX;
                    if (i <= STATIONARY) {
                        p = 0.5 * wc + 2.0;
                        wc = -0.5 / p;
                    }
                    const double d = ((double)x[i + 1] - 2.0 * (double)x[i]) + (double)x[i - 1];
                    uu = (3.0 * d - 0.5 * uu) / p;
                    if (i >= lo) w2[i] = uu;
                }
            }
            everybody();
            // w2[i] = w2[i] * w2[i + 1] + u[i] from the far end down: first the value above the chunk, from u alone
            double W = 0.0;
            if (lo < hi && hi < n - 1) {
                const int e = hi + WARM < n - 1 ? hi + WARM : n - 1;
                for (int i = e - 1; i >= hi; --i) W = forward_coef(i) * W + w2[i];
            }
            everybody();
            for (int i = hi - 1; i >= lo; --i) {
                W = forward_coef(i) * W + w2[i];
                w2[i] = W;
            }
            everybody();
        }
    }

    switch (mode) {
        case 'l': write_row<T, 'l', V, G>(out, x, w2, n, m, mode, tid); break;
        case 'h': write_row<T, 'h', V, G>(out, x, w2, n, m, mode, tid); break;
        case 's': write_row<T, 's', V, G>(out, x, w2, n, m, mode, tid); break;
        default: write_row<T, STEP, V, G>(out, x, w2, n, m, mode, tid); break;
    }
}

template <typename T, typename IN>
void launch_interp(const InterpArgs* A, int64_t n_wf, int vec, int lds_bytes, hipStream_t stream) {
#define DSP_INTERP_LAUNCH(NV, WIDE, OV, BLOCKS) \
    hipLaunchKernelGGL((dsp_interp_kernel<T, IN, NV, WIDE, OV>), dim3(BLOCKS), dim3(256), lds_bytes, stream, *A, n_wf)
#define DSP_INTERP_LAUNCH_OV(NV, WIDE, BLOCKS)       \
    if (A->out_vec)                                  \
        DSP_INTERP_LAUNCH(NV, WIDE, true, BLOCKS);   \
    else                                             \
        DSP_INTERP_LAUNCH(NV, WIDE, false, BLOCKS)
    if (A->wide) {
        if (vec) {
            DSP_INTERP_LAUNCH_OV(RowVec<IN>::N, true, (unsigned)n_wf);
        } else {
            DSP_INTERP_LAUNCH_OV(1, true, (unsigned)n_wf);
        }
    } else {
        if (vec) {
            DSP_INTERP_LAUNCH_OV(RowVec<IN>::N, false, row_blocks(n_wf));
        } else {
            DSP_INTERP_LAUNCH_OV(1, false, row_blocks(n_wf));
        }
    }
#undef DSP_INTERP_LAUNCH_OV
#undef DSP_INTERP_LAUNCH
}

}  // namespace

template <typename T, typename IN>
int set_lds(int lds_bytes) {
    const void* kernels[] = {reinterpret_cast<const void*>(&dsp_interp_kernel<T, IN, RowVec<IN>::N, true, true>),
                             reinterpret_cast<const void*>(&dsp_interp_kernel<T, IN, RowVec<IN>::N, true, false>),
                             reinterpret_cast<const void*>(&dsp_interp_kernel<T, IN, 1, true, true>),
                             reinterpret_cast<const void*>(&dsp_interp_kernel<T, IN, 1, true, false>)};
    for (const void* k : kernels)
        if (int rc = (int)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes)) return rc;
    return 0;
}

extern "C" int dsp_internal_set_interp_lds(int dtype, int lds_bytes) {
    switch (dtype) {
        case DSP_F32: return set_lds<float, float>(lds_bytes);
        case DSP_I16: return set_lds<float, int16_t>(lds_bytes);
        case DSP_U16: return set_lds<float, uint16_t>(lds_bytes);
        default: return set_lds<double, double>(lds_bytes);
    }
}

extern "C" int dsp_internal_launch_interp(const InterpArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream) {
    (void)err;  // (no row of this kernel is a DSPFatal)
    if (n_wf <= 0) return 0;
    const int esz = dtype == DSP_F64 ? 8 : 4;
    // (the planner's bounds, once more where the LDS is sized and the index rules divide)
    if (!dsp_interp::mode_ok(A->mode) || A->len < 1 || A->len > dsp_interp::max_len(A->mode, esz) || A->out_len < 1 || (A->mode == 'h' && A->len < 2) ||
        (A->mode == 'i' && A->out_len % A->len != 0) || A->wide != (dsp_interp::wide(A->mode, A->len, esz) ? 1 : 0) || n_wf > 0x7fffffff)
        return (int)hipErrorInvalidValue;
    const int lds = dsp_interp::lds_bytes(A->mode, A->len, esz);
    switch (dtype) {
        case DSP_F32: launch_interp<float, float>(A, n_wf, vec, lds, stream); break;
        case DSP_I16: launch_interp<float, int16_t>(A, n_wf, vec, lds, stream); break;
        case DSP_U16: launch_interp<float, uint16_t>(A, n_wf, vec, lds, stream); break;
        case DSP_F64: launch_interp<double, double>(A, n_wf, vec, lds, stream); break;
        default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}
