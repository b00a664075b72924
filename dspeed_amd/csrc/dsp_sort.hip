// dsp_sort.hip -- sort (processors/sort.py:36-42): every row in ascending order, -inf first and +inf last; a row that holds a NaN comes
// out as NaNs.  -0.0 sorts before +0.0 (the total order of the bit patterns; NumPy leaves their order open).
//
// One row is P = dsp_sort::padded(n) unsigned keys in LDS (dsp_kernels.h, dsp_sort: the key map, the geometry, the schedule), sorted by a
// bitonic network and mapped back on the way out.
//   geometry   rows of P <= NARROW_MAX keys get a wavefront each, four to a workgroup, and need no barrier; longer ones a workgroup of
//              256.  Both are this one kernel: WIDE chooses what "everybody" means.  A wide row's four wavefronts agree on "a NaN" through
//              one word behind the keys (16 bytes past the 64 KiB of the longest rows: dsp_internal_set_sort_lds).
//   staging    the shared loader (dsp_row_stream.h): 16 bytes per lane and load where start, stride and length allow, else a sample per
//              lane.  Samples become keys as they arrive -- integer min / max is then the compare-exchange and the NaN test one
//              unsigned comparison -- and the keys from n to P are +inf's: they tie with real +inf samples and stay behind sample n - 1.
//   tile pass  a wavefront takes a tile of 512 keys into registers, a chunk of 8 neighbours per lane, and runs every step whose stride is
//              below 512 there: strides 4, 2, 1 inside the chunk, strides 8 .. 256 against the lane 1 .. 32 away (quad permutes for 1 and
//              2, ds_swizzle for 4, 8, 16, ds_bpermute for 32: the LDS crossbar, no LDS memory).  The first tile pass runs stages 2 .. 512
//              whole; every longer stage k runs its steps of stride k / 2 .. 512 on pairs in LDS, a pair per thread and turn, and ends
//              with a tile pass.  A lane's chunk is 32 or 64 bytes of LDS, read and written 16 bytes at a time, every lane its slots
//              in the same order: chunks 2 or 4 slots apart put two or four lanes of a group on a slot, and an order staggered by lane
//              that avoids it was measured 2 to 3 % slower at 1024 and 8192 samples (its selects cost more than the conflicts).
//   counts     per row, derived from this code and the schedule, not measured (dsp_sort::lds_passes; a pass reads and writes all P keys
//              once; vector instructions per wavefront and tile or turn as the code is written, selects included, address arithmetic
//              not): a compare-exchange in registers is 4 (min, max, two selects), one across lanes 4 per key (the move, min, max, a
//              select), one in LDS 4 and its two reads and two writes.
//                1024 float32 samples   P = 1024, 2 tiles: the staging write, 3 passes (stages 2 .. 512; stride 512; strides 256 .. 1 of
//                                       stage 1024), the read on the way out.  Tile passes: 24 register steps of 16 and 21 cross-lane steps
//                                       of 32 in the first, 3 and 6 in the second, each on 2 tiles: 2 (384 + 672) + 2 (48 + 192) = 2592
//                                       instructions per row; the LDS step 8 turns of 4: 32.  About 2600, a wavefront's.
//                8192 float32 samples   P = 8192, 16 tiles over 4 wavefronts: the staging write, 15 passes (1 + 2 + 3 + 4 + 5: ten of them
//                                       LDS steps, five tile passes), the read on the way out.  16 (1056) + 4 x 16 (240) = 32 256 in tile
//                                       passes, 10 LDS steps of 64 turns of 4: 2560.  About 34 800 over the four wavefronts, with a
//                                       barrier behind each of the 15 passes.
#include <hip/hip_runtime.h>

#include "dsp_kernels.h"
#include "dsp_launch.h"
#include "dsp_row_stream.h"
#include "dsp_wave.h"

namespace {

using namespace dsp_sort;

template <typename T>
struct KeyOf;
template <>
struct KeyOf<float> {
    typedef uint32_t U;
    static constexpr U POS_INF = KEY_POS_INF32;
    static __device__ __forceinline__ U bits(float v) { return __float_as_uint(v); }
    static __device__ __forceinline__ float value(U b) { return __uint_as_float(b); }
};
template <>
struct KeyOf<double> {
    typedef uint64_t U;
    static constexpr U POS_INF = KEY_POS_INF64;
    static __device__ __forceinline__ U bits(double v) { return (U)__double_as_longlong(v); }
    static __device__ __forceinline__ double value(U b) { return __longlong_as_double((long long)b); }
};

// the key of the lane M away (lane ^ M), M a power of two below 64
template <int M>
__device__ __forceinline__ uint32_t lane_xor(uint32_t v) {
    if constexpr (M == 1)
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true);  // quad_perm [1, 0, 3, 2]
    else if constexpr (M == 2)
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true);  // quad_perm [2, 3, 0, 1]
    else if constexpr (M < 32)
        return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x1f | (M << 10));  // bit-mask mode: and 0x1f, or 0, xor M, within 32 lanes
    else
        return (uint32_t)__builtin_amdgcn_ds_bpermute((lane_id() ^ M) << 2, (int)v);
}
template <int M>
__device__ __forceinline__ uint64_t lane_xor(uint64_t v) {
    return (uint64_t)lane_xor<M>((uint32_t)(v >> 32)) << 32 | lane_xor<M>((uint32_t)v);
}

template <typename U>
__device__ __forceinline__ U umin(U a, U b) {
    return a < b ? a : b;
}
template <typename U>
__device__ __forceinline__ U umax(U a, U b) {
    return a < b ? b : a;
}

// step (k, J) on a lane's chunk, J < CHUNK; `base` is the index of key[0]
template <int J, typename U>
__device__ __forceinline__ void chunk_step(U (&key)[CHUNK], int base, int k) {
#pragma unroll
    for (int r = 0; r < CHUNK; ++r) {
        if (r & J) continue;
        const U lo = umin(key[r], key[r | J]), hi = umax(key[r], key[r | J]);
        const bool up = ascends(base | r, k);  // (k >= CHUNK: the lane's, one comparison for all of them)
        key[r] = up ? lo : hi;
        key[r | J] = up ? hi : lo;
    }
}

// step (k, CHUNK M) of a tile: against the chunk of the lane M away
template <int M, typename U>
__device__ __forceinline__ void lane_step(U (&key)[CHUNK], int base, int k) {
    const bool smaller = keeps_min(base, k, CHUNK * M);
#pragma unroll
    for (int r = 0; r < CHUNK; ++r) {
        const U other = lane_xor<M>(key[r]);
        key[r] = smaller ? umin(key[r], other) : umax(key[r], other);
    }
}

// the steps of stages k_lo .. k_hi whose stride is below TILE, on the tile whose chunk `base` starts this lane's
template <typename U>
__device__ __forceinline__ void tile_steps(U (&key)[CHUNK], int base, int k_lo, int k_hi) {
    for (int k = k_lo; k <= k_hi; k <<= 1) {  // (k is the wavefront's: the branches are scalar)
        if (k >= 64 * CHUNK) lane_step<32>(key, base, k);
        if (k >= 32 * CHUNK) lane_step<16>(key, base, k);
        if (k >= 16 * CHUNK) lane_step<8>(key, base, k);
        if (k >= 8 * CHUNK) lane_step<4>(key, base, k);
        if (k >= 4 * CHUNK) lane_step<2>(key, base, k);
        if (k >= 2 * CHUNK) lane_step<1>(key, base, k);
        if (k >= 8) chunk_step<4>(key, base, k);
        if (k >= 4) chunk_step<2>(key, base, k);
        chunk_step<1>(key, base, k);
    }
}

// N: samples per lane and load (dsp_row_stream.h); WIDE: a workgroup per row, else a wavefront
template <typename T, typename IN, int N, bool WIDE>
__global__ void __launch_bounds__(256) dsp_sort_kernel(SortArgs A, int64_t n_wf) {
    typedef typename KeyOf<T>::U U;
    typedef U Slot __attribute__((ext_vector_type(16 / sizeof(U))));  // 16 bytes of keys
    static_assert(CHUNK == 8, "tile_steps is written for chunks of 8");
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int K = N > 1 ? 4 : 8;        // loads in flight
    constexpr int G = WIDE ? 256 : 64;      // threads of a row
    constexpr int NW = WIDE ? 4 : 1;        // wavefronts of a row
    constexpr int PER = 16 / sizeof(U), SLOTS = CHUNK / PER;  // keys per 16 bytes, 16-byte slots per chunk
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const int tid = WIDE ? (int)threadIdx.x : lane;
    const int64_t row = WIDE ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + wave;
    if (!WIDE && row >= n_wf) return;  // (whole wavefronts, and no barrier in this geometry; WIDE: the grid is n_wf)
    const int n = A.len, P = A.padded;
    U* keys = (U*)lds_raw + (WIDE ? 0 : wave * P);
    int* row_bad = (int*)((U*)lds_raw + P);  // (WIDE)
    const IN* w = (const IN*)A.wf + row * A.wf_stride + A.wf_offset;
    auto everybody = [&]() {
        if constexpr (WIDE)
            __syncthreads();
        else
            wave_sync();
    };

    // staging
    if constexpr (WIDE) {
        if (tid == 0) *row_bad = 0;
        __syncthreads();
    }
    for (int i = n + tid; i < P; i += G) keys[i] = KeyOf<T>::POS_INF;
    bool bad = false;
    for (int g0 = (WIDE ? wave : 0) * K; g0 < row_groups<N>(n); g0 += NW * K) {
        T x[K][N];
        load_row_groups<T, IN, N, K>(x, w, n, g0, lane);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int s = in_row<N>(g0, k, 0, lane);
            if (s >= n) continue;  // (n is a multiple of N: a vector that starts inside the row lies inside it whole)
            U key[N];
#pragma unroll
            for (int j = 0; j < N; ++j) {
                key[j] = key_of(KeyOf<T>::bits(x[k][j]));
                bad |= key_is_nan(key[j]);
            }
            if constexpr (N > 1) {  // 16 bytes of keys a store (N is 1 or 2 slots' worth)
                static_assert(N % PER == 0, "whole slots");
#pragma unroll
                for (int q = 0; q < N / PER; ++q) {
                    Slot v;
#pragma unroll
                    for (int e = 0; e < PER; ++e) v[e] = key[q * PER + e];
                    ((Slot*)(keys + s))[q] = v;
                }
            } else {
                keys[s] = key[0];
            }
        }
    }
    bad = wave_any(bad);
    if constexpr (WIDE) {
        if (bad && lane == 0) *row_bad = 1;
        __syncthreads();  // (also the barrier behind the staging)
        bad = *row_bad != 0;
    } else {
        wave_sync();
    }

    T* out = (T*)A.out + row * A.out_stride;
    if (bad) {
        const T nanv = quiet_nan<T>();
        for (int i = tid; i < n; i += G) out[i] = nanv;
        return;  // (everybody of the row: `bad` is the row's)
    }

    // a tile pass: every lane of a wavefront runs the steps (they exchange with each other); lanes past a short row hold +inf's and store nothing
    auto tile_pass = [&](int k_lo, int k_hi) {
        for (int t0 = (WIDE ? wave : 0) * TILE; t0 < P; t0 += NW * TILE) {
            const int base = t0 + lane * CHUNK;
            U key[CHUNK];
            Slot* at = (Slot*)(keys + base);
#pragma unroll
            for (int q = 0; q < SLOTS; ++q) {
                Slot v = (Slot)(KeyOf<T>::POS_INF);
                if (base < P) v = at[q];
#pragma unroll
                for (int e = 0; e < PER; ++e) key[q * PER + e] = v[e];
            }
            tile_steps(key, base, k_lo, k_hi);
            if (base < P) {
#pragma unroll
                for (int q = 0; q < SLOTS; ++q) {
                    Slot v;
#pragma unroll
                    for (int e = 0; e < PER; ++e) v[e] = key[q * PER + e];
                    at[q] = v;
                }
            }
        }
        everybody();
    };

    tile_pass(2, P < TILE ? P : TILE);
    for (int k = 2 * TILE; k <= P; k <<= 1) {
        for (int j = k >> 1; j >= TILE; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += G) {
                const int low = t & (j - 1), i = ((t - low) << 1) | low;
                const U a = keys[i], b = keys[i + j];
                const bool up = ascends(i, k);
                keys[i] = up ? umin(a, b) : umax(a, b);
                keys[i + j] = up ? umax(a, b) : umin(a, b);
            }
            everybody();
        }
        tile_pass(k, k);
    }

    // the row: coalesced scalar stores (rows of any length keep no alignment)
    for (int i = tid; i < n; i += G) out[i] = KeyOf<T>::value(bits_of(keys[i]));
}

template <typename T, typename IN>
void launch_sort(const SortArgs* A, int64_t n_wf, int vec, int lds_bytes, hipStream_t stream) {
#define DSP_SORT_LAUNCH(NV, WIDE, BLOCKS) \
    hipLaunchKernelGGL((dsp_sort_kernel<T, IN, NV, WIDE>), dim3(BLOCKS), dim3(256), lds_bytes, stream, *A, n_wf)
    if (A->wide) {
        if (vec)
            DSP_SORT_LAUNCH(RowVec<IN>::N, true, (unsigned)n_wf);
        else
            DSP_SORT_LAUNCH(1, true, (unsigned)n_wf);
    } else {
        if (vec)
            DSP_SORT_LAUNCH(RowVec<IN>::N, false, row_blocks(n_wf));
        else
            DSP_SORT_LAUNCH(1, false, row_blocks(n_wf));
    }
#undef DSP_SORT_LAUNCH
}

}  // namespace

template <typename T, typename IN>
int set_lds(int lds_bytes) {
    int rc = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(&dsp_sort_kernel<T, IN, RowVec<IN>::N, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (rc) return rc;
    return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(&dsp_sort_kernel<T, IN, 1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
}

extern "C" int dsp_internal_set_sort_lds(int dtype, int lds_bytes) {
    switch (dtype) {
        case DSP_F32: return set_lds<float, float>(lds_bytes);
        case DSP_I16: return set_lds<float, int16_t>(lds_bytes);
        case DSP_U16: return set_lds<float, uint16_t>(lds_bytes);
        default: return set_lds<double, double>(lds_bytes);
    }
}

extern "C" int dsp_internal_launch_sort(const SortArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream) {
    (void)err;  // (no row of this kernel is a DSPFatal)
    if (n_wf <= 0) return 0;
    const int esz = dtype == DSP_F64 ? 8 : 4;
    // (the planner's bounds, once more where the LDS is sized: the padded length the plan names is the row's, and a workgroup's 64 KiB hold it)
    if (A->len < 1 || A->len > DSP_SORT_F32_MAX / (esz / 4) || A->padded != dsp_sort::padded(A->len) || A->wide != (dsp_sort::wide(A->len) ? 1 : 0) ||
        n_wf > 0x7fffffff)
        return (int)hipErrorInvalidValue;
    const int lds = dsp_sort::lds_bytes(A->len, esz);
    switch (dtype) {
        case DSP_F32: launch_sort<float, float>(A, n_wf, vec, lds, stream); break;
        case DSP_I16: launch_sort<float, int16_t>(A, n_wf, vec, lds, stream); break;
        case DSP_U16: launch_sort<float, uint16_t>(A, n_wf, vec, lds, stream); break;
        case DSP_F64: launch_sort<double, double>(A, n_wf, vec, lds, stream); break;
        default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}
