// dsp_lane_tiles.h -- how a kernel that gives a waveform to a LANE passes 64 rows through LDS, a tile of 64 rows x 64 samples at a time
// (dsp_kernels.h, dsp_pileup: ROWS, TS, PITCH).  Internal header.
//
// The tile is written along the rows and read along the columns: lane l walks row l of the tile, `tile + l * PITCH`.  Whole tiles of whole
// blocks are fetched with 16-byte loads -- V samples of a row per lane, V rows per instruction -- one tile ahead, in registers; the last
// rows of a batch, the last samples of a row and rows that are not whole vectors take the element-wise path.  A kernel of this kind runs
//     LaneTiles<T, InT, VEC> rows(tile, g, stride, r0, rows_here, n, lane);
//     rows.run([&](int s0, int w) { ... lane l reads (and may write over) tile[l * PITCH + u], u < w: samples s0 + u of row r0 + l ... });
// and may run it again for another pass over the same rows.  The body is entered behind a wave_sync and followed by one; a body that hands
// the tile on to other lanes (store_lane_tile) puts a wave_sync of its own in front.
#pragma once
#include <hip/hip_runtime.h>

#include "dsp_kernels.h"
#include "dsp_wave.h"

namespace {

// VEC: rows start on 16-byte boundaries, lie whole vectors apart and hold whole vectors (the planner's and the call's word)
template <typename T, typename InT, bool VEC>
struct LaneTiles {
    static constexpr int ROWS = dsp_pileup::ROWS, TS = dsp_pileup::TS, PITCH = dsp_pileup::PITCH;
    static constexpr int V = 16 / (int)sizeof(InT), NV = TS / V;  // samples per load, loads per lane and tile
    typedef InT vec_t __attribute__((ext_vector_type(V)));
    T* tile;
    const InT* __restrict__ g;
    int64_t stride, r0;
    int rows_here, n, lane;
    int pr, pc;  // row within a group of V rows, first sample of this lane's piece
    bool wide;
    vec_t pf[NV];

    __device__ __forceinline__ LaneTiles(T* tile_, const InT* g_, int64_t stride_, int64_t r0_, int rows_here_, int n_, int lane_)
        : tile(tile_), g(g_), stride(stride_), r0(r0_), rows_here(rows_here_), n(n_), lane(lane_), pr(lane_ / (TS / V)), pc((lane_ % (TS / V)) * V),
          wide(VEC && rows_here_ == ROWS) {}

    __device__ __forceinline__ void fetch(int s0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) pf[q] = *(const vec_t*)(g + (r0 + q * V + pr) * stride + s0 + pc);
    }
    __device__ __forceinline__ void commit() {
#pragma unroll
        for (int q = 0; q < NV; ++q)
#pragma unroll
            for (int e = 0; e < V; ++e) tile[(q * V + pr) * PITCH + pc + e] = (T)pf[q][e];
    }

    template <typename Body>
    __device__ __forceinline__ void run(Body&& body) {
        if (wide && n >= TS) fetch(0);
        for (int s0 = 0; s0 < n; s0 += TS) {
            const int w = n - s0 < TS ? n - s0 : TS;
            if (wide && w == TS) {
                commit();
                if (s0 + 2 * TS <= n) fetch(s0 + TS);
            } else {
#pragma unroll 8
                for (int r = 0; r < rows_here; ++r) tile[r * PITCH + lane] = lane < w ? (T)g[(r0 + r) * stride + s0 + lane] : (T)0;
            }
            wave_sync();
            body(s0, w);
            wave_sync();
        }
    }
};

// samples [s0, s0 + w) of the tile's rows go to `outp`, rows out_stride apart: 16 bytes a lane for a whole tile of a whole block where the
// output rows are whole vectors (`wide_out`: the call's word and rows_here == 64), element-wise otherwise
template <typename T>
__device__ __forceinline__ void store_lane_tile(const T* tile, T* __restrict__ outp, int64_t out_stride, int64_t r0, int rows_here, int s0, int w, int lane,
                                                bool wide_out) {
    constexpr int TS = dsp_pileup::TS, PITCH = dsp_pileup::PITCH;
    constexpr int VO = 16 / (int)sizeof(T), NVO = TS / VO;
    typedef T ovec_t __attribute__((ext_vector_type(VO)));
    const int por = lane / (TS / VO), poc = (lane % (TS / VO)) * VO;
    if (wide_out && w == TS) {
#pragma unroll
        for (int q = 0; q < NVO; ++q) {
            ovec_t o;
#pragma unroll
            for (int e = 0; e < VO; ++e) o[e] = tile[(q * VO + por) * PITCH + poc + e];
            *(ovec_t*)(outp + (r0 + q * VO + por) * out_stride + s0 + poc) = o;
        }
    } else {
#pragma unroll 8
        for (int r = 0; r < rows_here; ++r)
            if (lane < w) outp[(r0 + r) * out_stride + s0 + lane] = tile[r * PITCH + lane];
    }
}

// rows of n values that turned out NaN rows behind their last tile (`nan_rows`: a bit per row of the block) are written over, once the
// stores before are done
template <typename T>
__device__ __forceinline__ void overwrite_nan_rows(unsigned long long nan_rows, T* __restrict__ outp, int64_t out_stride, int64_t r0, int rows_here, int n, int lane) {
    if (!nan_rows) return;
    const T nanv = quiet_nan<T>();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int r = 0; r < rows_here; ++r)
        if ((nan_rows >> r) & 1ull)
            for (int k = lane; k < n; k += 64) outp[(r0 + r) * out_stride + k] = nanv;
}

}  // namespace
