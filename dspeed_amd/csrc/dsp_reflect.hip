// dsp_reflect.hip -- reflected_convolve_wf (processors/convolutions.py:122-182): every row of n samples convolved with one kernel of
// m <= n taps, the row continued past both ends by its mirror image (numpy's "reflect": the edge sample is not repeated), n outputs.  A
// row that holds a NaN comes out as NaNs, and so does every row when the kernel holds one.  With an avg_current of the filtered row in
// the program, that runs in the same launch: the filtered row need not go to memory and back.
//
// The index rule and the layout of the staged row are dsp_kernels.h's, dsp_reflect, shared with the planner and tests/reflect_index.cpp.
//   geometry   rows of up to 8 KiB staged get a wavefront each, four to a workgroup, and need no barrier; longer ones a workgroup of 256.
//              Both are this one kernel: WIDE chooses what "everybody" means.  A wide row's wavefronts agree on "a NaN" through one word
//              behind the row (dsp_internal_set_reflect_lds raises the limit for the longest rows).
//   staging    the shared loader (dsp_row_stream.h) into LDS, in the loop's type; the NaN screen happens here.  A sample that the mirror
//              shows is written twice (or three times: at m == n the first and last margins overlap in the row), so that the row stands
//              in LDS with left(m) mirrored samples ahead of it and right(m) behind it and the inner loop has no branch.
//   inner loop a lane makes V = 16 bytes' worth of consecutive outputs.  It walks the taps in ascending order, V a step; a step reads one
//              16-byte vector of samples -- lanes 16 bytes apart: conflict free -- and keeps the previous one, so R + m - 1 samples (rounded
//              up to vectors) are read for R outputs.  The taps are the same for every lane: loads from the constant address space, which
//              the compiler issues on the scalar unit.
//   arithmetic one float64 accumulator per output from +0, the products added in ascending k, one rounding at the store.  In the float32
//              loop the product of two float32 values is exact in float64, so the fused multiply-add used there is the multiply and the
//              add; the float64 loop multiplies and adds (the library is built with -ffp-contract=off).
//   stores     16 bytes per lane where the output rows' start and stride are whole vectors (ReflectArgs::out_vec) and the lane's outputs
//              lie inside the row whole, else a sample per lane; non-temporal: the row is not read again.
//   avg_current (ReflectArgs::lag > 0)  a lane keeps its outputs in registers until everybody of the row has made theirs of this turn, then
//              writes them over the raw samples, which no later turn reads: output i goes to position i of the LDS row, below everything
//              outputs above i read.  Behind the last turn curr[k] = (g[k + lag] - g[k]) / length in the loop's type, the expression and
//              rounding of DSP_OP_AVG_CURRENT; a filtered row with a NaN in it (an infinite sample under the kernel) gives NaNs, as a
//              row with a NaN does there.
#include <hip/hip_runtime.h>

#include "dsp_kernels.h"
#include "dsp_launch.h"
#include "dsp_row_stream.h"
#include "dsp_wave.h"

namespace {

using namespace dsp_reflect;

// acc + a * b: exact products in the float32 loop (one instruction), a multiply and an add in the float64 loop
template <typename T>
__device__ __forceinline__ double mac(double acc, double a, double b) {
    if constexpr (sizeof(T) == 4)
        return __builtin_fma(a, b, acc);
    else
        return acc + a * b;
}

// N: samples per lane and load (dsp_row_stream.h); WIDE: a workgroup per row, else a wavefront; OV: 16-byte stores of the filtered row
template <typename T, typename IN, int N, bool WIDE, bool OV>
__global__ void __launch_bounds__(256) dsp_reflect_kernel(ReflectArgs A, int64_t n_wf) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    typedef T Vec __attribute__((ext_vector_type(16 / sizeof(T))));
    typedef const T __attribute__((address_space(4))) * Taps;  // uniform, read-only for the launch: scalar loads
    constexpr int K = N > 1 ? 4 : 8;    // loads in flight
    constexpr int G = WIDE ? 256 : 64;  // threads of a row
    constexpr int NW = WIDE ? 4 : 1;    // wavefronts of a row
    constexpr int V = vec((int)sizeof(T));
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const int tid = WIDE ? (int)threadIdx.x : lane;
    const int64_t row = WIDE ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + wave;
    if (!WIDE && row >= n_wf) return;  // (whole wavefronts, and no barrier in this geometry; WIDE: the grid is n_wf)
    const int n = A.len, m = A.n_taps, lag = A.lag;
    const int rb = row_bytes(n, m, (int)sizeof(T));
    const int M = m + pad(m, (int)sizeof(T));  // a multiple of V: the staged row starts pad samples in
    T* e = (T*)(lds_raw + (WIDE ? 0 : wave * rb));
    T* x = e + (M - m) + left(m);       // sample 0 of the row
    int* row_flags = (int*)(lds_raw + rb);  // (WIDE) bit 0: a NaN in the row, bit 1: in the filtered row
    const IN* w = (const IN*)A.wf + row * A.wf_stride + A.wf_offset;
    const Taps taps = (Taps)(uintptr_t)A.taps;
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
    bool bad = false;
    const int mirror_hi = left(m), mirror_lo = n - 1 - right(m);  // samples 1 .. mirror_hi stand ahead of the row too, mirror_lo .. n - 2 behind it
    for (int g0 = (WIDE ? wave : 0) * K; g0 < row_groups<N>(n); g0 += NW * K) {
        T s[K][N];
        load_row_groups<T, IN, N, K>(s, w, n, g0, lane);
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const int at = in_row<N>(g0, k, j, lane);
                if (at >= n) continue;
                const T v = s[k][j];
                bad |= v != v;
                x[at] = v;
                if (at >= 1 && at <= mirror_hi) x[-at] = v;
                if (at >= mirror_lo && at <= n - 2) x[2 * (n - 1) - at] = v;
            }
        }
    }
    bad = wave_any(bad);
    if constexpr (WIDE) {
        if (bad && lane == 0) atomicOr(row_flags, 1);
        __syncthreads();  // (also the barrier behind the staging)
        bad = (*row_flags & 1) != 0;
    } else {
        wave_sync();
    }
    bad |= A.taps_nan != 0;

    T* out = A.out ? (T*)A.out + row * A.out_stride : nullptr;
    T* cur = lag > 0 ? (T*)A.cur + row * A.cur_stride : nullptr;
    const int nc = n - lag;
    if (bad) {
        const T nanv = quiet_nan<T>();
        if (out)
            for (int i = tid; i < n; i += G) out[i] = nanv;
        if (cur)
            for (int i = tid; i < nc; i += G) cur[i] = nanv;
        return;  // (everybody of the row: `bad` is the row's)
    }

    // the outputs: thread `tid` of G takes V consecutive ones a turn
    bool g_nan = false;
    for (int turn = 0; turn < n; turn += G * V) {
        const int i0 = turn + tid * V;
        T g[V];
#pragma unroll
        for (int r = 0; r < V; ++r) g[r] = (T)0;
        if (i0 < n) {
            double acc[V], win[2 * V];  // win: the samples at i0 + M - k0 - V .. + 2 V - 1 of the LDS row, as float64
#pragma unroll
            for (int r = 0; r < V; ++r) acc[r] = 0.0;
            {
                const Vec q = *(const Vec*)(e + i0 + M);
#pragma unroll
                for (int r = 0; r < V; ++r) win[r] = (double)q[r];
            }
            for (int k0 = 0; k0 < m; k0 += V) {
                const Vec q = *(const Vec*)(e + i0 + M - k0 - V);
#pragma unroll
                for (int r = 0; r < V; ++r) {
                    win[V + r] = win[r];
                    win[r] = (double)q[r];
                }
                if (k0 + V <= m) {
#pragma unroll
                    for (int t = 0; t < V; ++t) {
                        const double c = (double)taps[k0 + t];
#pragma unroll
                        for (int r = 0; r < V; ++r) acc[r] = mac<T>(acc[r], win[V - 1 - t + r], c);
                    }
                } else {  // the last taps of a kernel whose length is no multiple of V (no product with what lies below the staged row: 0 x inf)
#pragma unroll
                    for (int t = 0; t < V - 1; ++t) {
                        if (k0 + t >= m) break;
                        const double c = (double)taps[k0 + t];
#pragma unroll
                        for (int r = 0; r < V; ++r) acc[r] = mac<T>(acc[r], win[V - 1 - t + r], c);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < V; ++r) {
                g[r] = (T)acc[r];
                g_nan |= i0 + r < n && g[r] != g[r];
            }
            if (out) {
                bool whole = false;
                if constexpr (OV) {
                    if (i0 + V <= n) {
                        Vec q;
#pragma unroll
                        for (int r = 0; r < V; ++r) q[r] = g[r];
                        __builtin_nontemporal_store(q, (Vec*)(out + i0));
                        whole = true;
                    }
                }
                if (!whole) {
#pragma unroll
                    for (int r = 0; r < V; ++r)
                        if (i0 + r < n) __builtin_nontemporal_store(g[r], out + i0 + r);
                }
            }
        }
        if (lag > 0) {
            everybody();  // nobody reads the samples of this turn's outputs any more; later turns read above them
            if (i0 < n) {
                Vec q;
#pragma unroll
                for (int r = 0; r < V; ++r) q[r] = g[r];
                *(Vec*)(e + i0) = q;
            }
        }
    }
    if (lag <= 0) return;

    // avg_current of the filtered row, which now stands at e[0 .. n)
    g_nan = wave_any(g_nan);
    if constexpr (WIDE) {
        if (g_nan && lane == 0) atomicOr(row_flags, 2);
        __syncthreads();  // (also the barrier behind the last turn)
        g_nan = (*row_flags & 2) != 0;
    } else {
        wave_sync();
    }
    const T length = (T)A.length;
    for (int k = tid; k < nc; k += G) {
        const T v = g_nan ? quiet_nan<T>() : (T)(e[k + lag] - e[k]) / length;
        __builtin_nontemporal_store(v, cur + k);
    }
}

template <typename T, typename IN>
void launch_reflect(const ReflectArgs* A, int64_t n_wf, int vec, int lds_bytes, hipStream_t stream) {
#define DSP_REFLECT_LAUNCH(NV, WIDE, OV, BLOCKS) \
    hipLaunchKernelGGL((dsp_reflect_kernel<T, IN, NV, WIDE, OV>), dim3(BLOCKS), dim3(256), lds_bytes, stream, *A, n_wf)
#define DSP_REFLECT_LAUNCH_OV(NV, WIDE, BLOCKS)      \
    if (A->out_vec)                                  \
        DSP_REFLECT_LAUNCH(NV, WIDE, true, BLOCKS);  \
    else                                             \
        DSP_REFLECT_LAUNCH(NV, WIDE, false, BLOCKS)
    if (A->wide) {
        if (vec) {
            DSP_REFLECT_LAUNCH_OV(RowVec<IN>::N, true, (unsigned)n_wf);
        } else {
            DSP_REFLECT_LAUNCH_OV(1, true, (unsigned)n_wf);
        }
    } else {
        if (vec) {
            DSP_REFLECT_LAUNCH_OV(RowVec<IN>::N, false, row_blocks(n_wf));
        } else {
            DSP_REFLECT_LAUNCH_OV(1, false, row_blocks(n_wf));
        }
    }
#undef DSP_REFLECT_LAUNCH_OV
#undef DSP_REFLECT_LAUNCH
}

}  // namespace

template <typename T, typename IN>
int set_lds(int lds_bytes) {
    const void* kernels[] = {reinterpret_cast<const void*>(&dsp_reflect_kernel<T, IN, RowVec<IN>::N, true, true>),
                             reinterpret_cast<const void*>(&dsp_reflect_kernel<T, IN, RowVec<IN>::N, true, false>),
                             reinterpret_cast<const void*>(&dsp_reflect_kernel<T, IN, 1, true, true>),
                             reinterpret_cast<const void*>(&dsp_reflect_kernel<T, IN, 1, true, false>)};
    for (const void* k : kernels)
        if (int rc = (int)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes)) return rc;
    return 0;
}

extern "C" int dsp_internal_set_reflect_lds(int dtype, int lds_bytes) {
    switch (dtype) {
        case DSP_F32: return set_lds<float, float>(lds_bytes);
        case DSP_I16: return set_lds<float, int16_t>(lds_bytes);
        case DSP_U16: return set_lds<float, uint16_t>(lds_bytes);
        default: return set_lds<double, double>(lds_bytes);
    }
}

extern "C" int dsp_internal_launch_reflect(const ReflectArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream) {
    (void)err;  // (no row of this kernel is a DSPFatal)
    if (n_wf <= 0) return 0;
    const int esz = dtype == DSP_F64 ? 8 : 4;
    // (the planner's bounds, once more where the LDS is sized and the margins are written)
    if (A->len < 1 || A->n_taps < 1 || A->n_taps > A->len || !dsp_reflect::fits(A->len, A->n_taps, esz) ||
        A->wide != (dsp_reflect::wide(A->len, A->n_taps, esz) ? 1 : 0) || !A->taps || A->lag < 0 || A->lag >= A->len || (A->lag > 0) != (A->cur != nullptr) ||
        (!A->out && !A->cur) || n_wf > 0x7fffffff)
        return (int)hipErrorInvalidValue;
    const int lds = dsp_reflect::lds_bytes(A->len, A->n_taps, esz);
    switch (dtype) {
        case DSP_F32: launch_reflect<float, float>(A, n_wf, vec, lds, stream); break;
        case DSP_I16: launch_reflect<float, int16_t>(A, n_wf, vec, lds, stream); break;
        case DSP_U16: launch_reflect<float, uint16_t>(A, n_wf, vec, lds, stream); break;
        case DSP_F64: launch_reflect<double, double>(A, n_wf, vec, lds, stream); break;
        default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}
