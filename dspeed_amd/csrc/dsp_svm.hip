// dsp_svm.hip -- svm_predict of processors/svm.py: the label a fitted scikit-learn SVC (libsvm, one-vs-one) gives every row, for the "rbf" and the
// "linear" kernel function.  What the pickle holds is a few constant arrays and what predict computes is GEMM-shaped, twice over:
//     G = X . SV^T        K = exp(-gamma (|x|^2 + |sv|^2 - 2 G))  (rbf)  or  G  (linear)        DEC = K . D + intercept        a vote
// with D (n_sv, P) the dual coefficients laid out per pair of classes on the host.  Both products run on the matrix cores in float64
// (v_mfma_f64_16x16x4_f64), as libsvm works in float64 on the row cast up; the model is float64 in both loops.
//   geometry   dsp_dense's tile of rows: a workgroup of 4 wavefronts takes 64 rows, a wavefront 16.  The support vectors come 64 at a time, four
//              accumulator tiles a wavefront; the decisions of a wavefront's rows stay in pair_blocks(P) accumulator tiles across all of them
//              (the kernel is built for 1, 4 and 16 blocks of 16 pairs).  Geometry and LDS layout are dsp_kernels.h's, dsp_svm, shared with
//              the planner.
//   transposed the first product is formed as G^T = SV . X^T: register r of a tile then holds, in lane l, support vector 4 r + (l >> 4) of the
//              tile against row l & 15 -- which is where the B operand of the NEXT instruction wants k = l >> 4 and column l & 15.  So K^T,
//              formed in place, feeds DEC^T += D^T . K^T from the registers: no pass through LDS between the products.  D's operand is
//              read from memory as it is needed (16 neighbouring pairs a support vector: 128 bytes), 0 beyond n_sv and beyond P.
//   staging    rows pass through LDS as float64, through the shared loader (dsp_row_stream.h), every wavefront its own 16 rows.  Rows of up
//              to RESIDENT_MAX samples are staged once, whole; longer ones in chunks of 32 samples, again for every block of support
//              vectors (they come from L2 then).  The support vectors' chunk is staged beside them by the whole workgroup.  Whatever lies
//              beyond n, beyond n_sv and beyond the batch is ZERO in LDS, in both operands: 0 x garbage may be NaN.
//   |x|^2      summed from the staged operand itself while the first block of support vectors is multiplied: every lane reads each sample
//              of its row & 15 once there; two exchanges across the lanes' quarters complete it.  |sv|^2 is the host's.  A negative
//              distance from cancellation counts as 0.
//   NaN rule   a row with a NaN gives a NaN label (svm.py:62-64) and NaN decisions: the NaN passes through both products, into every pair.
//              A row with an infinite sample gives the same (scikit-learn raises ValueError there; a kernel has no exception): its K may
//              be a finite 0, so such rows are flagged while they are summed.  The vote never turns a flagged row into a class.
//   vote       behind the last block the decisions, intercepts added, go to LDS, a row per lane of a wavefront's first 16: dec_p > 0 votes
//              for class i of the pair (i, j), anything else -- 0 too -- for j; the first class with the most votes wins; its value is
//              converted to the loop's type.
#include <hip/hip_runtime.h>

#include "dsp_kernels.h"
#include "dsp_launch.h"
#include "dsp_row_stream.h"
#include "dsp_wave.h"

namespace {

using namespace dsp_svm;

typedef double Acc __attribute__((ext_vector_type(4)));
// out[i][j] += sum_k a[i][k] b[k][j]: lane l hands in a[l & 15][l >> 4] and b[l >> 4][l & 15], register r of its result is out[(l >> 4) + 4 r][l & 15]
__device__ __forceinline__ Acc mma(double a, double b, Acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// N: samples per lane and load (dsp_row_stream.h); PB: blocks of 16 pairs a wavefront is built for
template <typename IN, typename OUT, int N, int PB>
__global__ void __launch_bounds__(256) dsp_svm_kernel(SvmArgs A, int64_t n_wf) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int RQ = 4;  // rows requested before the first is looked at
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6), tid = (int)threadIdx.x;
    const int n = A.len, n_sv = A.n_sv, P = A.n_pairs, pbu = pair_blocks(P), XP = x_pitch(n);
    const bool whole = resident(n), linear = A.linear != 0;
    double* xw = (double*)lds_raw + wave * WAVE_ROWS * XP;  // [WAVE_ROWS][XP]: this wavefront's rows
    double* svl = (double*)lds_raw + TILE_ROWS * XP;        // [SV_BLOCK][SV_PITCH]
    const int64_t row0 = (int64_t)blockIdx.x * TILE_ROWS + wave * WAVE_ROWS;
    const IN* w = (const IN*)A.wf + A.wf_offset;
    const int col = lane & 15, quarter = lane >> 4;

    Acc dec[PB];
#pragma unroll
    for (int b = 0; b < PB; ++b) dec[b] = Acc{0, 0, 0, 0};
    double nx = 0.0;  // |x|^2 of row `col`
    int bad = 0;      // ... and whether it holds a NaN or an infinity

    for (int sb = 0; sb < n_sv; sb += SV_BLOCK) {
        const bool first = sb == 0;
        Acc g[SV_TILES];
#pragma unroll
        for (int t = 0; t < SV_TILES; ++t) g[t] = Acc{0, 0, 0, 0};
        for (int k0 = 0; k0 < n; k0 += KC) {
            const int kc = n - k0 < KC ? n - k0 : KC;
            {  // the support vectors' chunk: a thread takes 8 neighbouring samples of one of them
                const int s = tid >> 2, part = (tid & 3) * 8;
                const bool in = sb + s < n_sv;
                const double* from = A.sv + (int64_t)(sb + s) * n + k0 + part;
                double v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = in && part + j < kc ? from[j] : 0.0;
#pragma unroll
                for (int j = 0; j < 8; ++j) svl[s * SV_PITCH + part + j] = v[j];
            }
            const int xo = whole ? k0 : 0;
            if (first || !whole) {
                // this wavefront's rows: the loader leaves 0 in the lanes beyond kc, and in every lane of a row beyond the batch
#pragma unroll
                for (int r0 = 0; r0 < WAVE_ROWS; r0 += RQ) {
                    double s[RQ][1][N];
#pragma unroll
                    for (int q = 0; q < RQ; ++q) {
                        const int64_t row = row0 + r0 + q;
                        load_row_groups<double, IN, N, 1>(s[q], w + row * A.wf_stride + k0, row < n_wf ? kc : 0, 0, lane);
                    }
                    const int at = lane * N;
                    if (at < KC) {
#pragma unroll
                        for (int q = 0; q < RQ; ++q)
#pragma unroll
                            for (int j = 0; j < N; ++j) xw[(r0 + q) * XP + xo + at + j] = s[q][0][j];
                    }
                }
            }
            __syncthreads();
            const int steps = (kc + DEPTH - 1) / DEPTH;
            for (int kk = 0; kk < steps; ++kk) {
                const int k = kk * DEPTH + quarter;
                const double x = xw[col * XP + xo + k];
                if (first) {
                    nx += x * x;
                    bad |= !(__builtin_fabs(x) < __builtin_inf());
                }
#pragma unroll
                for (int t = 0; t < SV_TILES; ++t)
                    if (sb + t * BLOCK < n_sv) g[t] = mma(svl[(t * BLOCK + col) * SV_PITCH + k], x, g[t]);
            }
            __syncthreads();
        }
        if (first) {  // the quarters of a row's sum
            nx += __shfl_xor(nx, 16);
            nx += __shfl_xor(nx, 32);
            bad |= __shfl_xor(bad, 16);
            bad |= __shfl_xor(bad, 32);
        }
#pragma unroll
        for (int t = 0; t < SV_TILES; ++t) {
            if (sb + t * BLOCK >= n_sv) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int sv = sb + t * BLOCK + 4 * r + quarter;
                const bool in = sv < n_sv;
                double kv = g[t][r];
                if (!linear) {
                    double d2 = nx + (in ? A.sv_norm[sv] : 0.0) - 2.0 * kv;
                    d2 = d2 < 0.0 ? 0.0 : d2;  // (a NaN stays one)
                    kv = exp(-A.gamma * d2);
                }
                if (!in) kv = 0.0;
                const double* drow = A.coef + (int64_t)sv * P;
#pragma unroll
                for (int b = 0; b < PB; ++b) {
                    if (b >= pbu) continue;
                    const int p = b * BLOCK + col;
                    dec[b] = mma(in && p < P ? drow[p] : 0.0, kv, dec[b]);
                }
            }
        }
    }

    // the decisions of this wavefront's rows, over the staging area (every wavefront is behind the last barrier of the loop)
    const int DP = dec_pitch(P);
    double* dl = (double*)lds_raw + wave * WAVE_ROWS * DP;  // [WAVE_ROWS][DP]
#pragma unroll
    for (int b = 0; b < PB; ++b) {
        if (b >= pbu) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = b * BLOCK + quarter + 4 * r;
            dl[col * DP + p] = dec[b][r] + (p < P ? A.intercept[p] : 0.0);
        }
    }
    __syncthreads();
    if (lane < WAVE_ROWS && row0 + lane < n_wf) {
        const double* d = dl + lane * DP;
        const int kcl = A.n_classes;
        bool nan = bad != 0;
        for (int p = 0; p < P; ++p) nan |= d[p] != d[p];
        int best = -1, best_c = 0;
        for (int c = 0; c < kcl; ++c) {
            int votes = 0;
            for (int j = c + 1; j < kcl; ++j) votes += d[pair(c, j, kcl)] > 0.0 ? 1 : 0;
            for (int i = 0; i < c; ++i) votes += d[pair(i, c, kcl)] > 0.0 ? 0 : 1;
            if (votes > best) best = votes, best_c = c;
        }
        ((OUT*)A.label)[(row0 + lane) * A.label_stride] = nan ? quiet_nan<OUT>() : (OUT)A.classes[best_c];
    }
    if (A.dec) {
        for (int r = 0; r < WAVE_ROWS; ++r) {
            const int64_t row = row0 + r;
            if (row >= n_wf) break;
            const int flagged = __shfl(bad, r);
            for (int p = lane; p < P; p += 64) A.dec[row * A.dec_stride + p] = flagged ? quiet_nan<double>() : dl[r * DP + p];
        }
    }
}

template <typename IN, typename OUT, int N>
void launch_svm_n(const SvmArgs* A, int64_t n_wf, int lds, hipStream_t stream) {
    const dim3 grid((unsigned)tiles(n_wf));
    switch (built_blocks(A->n_pairs)) {
        case 1: hipLaunchKernelGGL((dsp_svm_kernel<IN, OUT, N, 1>), grid, dim3(256), lds, stream, *A, n_wf); break;
        case 4: hipLaunchKernelGGL((dsp_svm_kernel<IN, OUT, N, 4>), grid, dim3(256), lds, stream, *A, n_wf); break;
        default: hipLaunchKernelGGL((dsp_svm_kernel<IN, OUT, N, PAIR_BLOCKS_MAX>), grid, dim3(256), lds, stream, *A, n_wf); break;
    }
}

template <typename IN, typename OUT>
void launch_svm(const SvmArgs* A, int64_t n_wf, int vec, int lds, hipStream_t stream) {
    if (vec)
        launch_svm_n<IN, OUT, RowVec<IN>::N>(A, n_wf, lds, stream);
    else
        launch_svm_n<IN, OUT, 1>(A, n_wf, lds, stream);
}

template <typename IN, typename OUT>
int set_lds(int lds_bytes) {
    const void* kernels[] = {reinterpret_cast<const void*>(&dsp_svm_kernel<IN, OUT, RowVec<IN>::N, 1>), reinterpret_cast<const void*>(&dsp_svm_kernel<IN, OUT, 1, 1>),
                             reinterpret_cast<const void*>(&dsp_svm_kernel<IN, OUT, RowVec<IN>::N, 4>), reinterpret_cast<const void*>(&dsp_svm_kernel<IN, OUT, 1, 4>),
                             reinterpret_cast<const void*>(&dsp_svm_kernel<IN, OUT, RowVec<IN>::N, PAIR_BLOCKS_MAX>),
                             reinterpret_cast<const void*>(&dsp_svm_kernel<IN, OUT, 1, PAIR_BLOCKS_MAX>)};
    for (const void* k : kernels)
        if (int rc = (int)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes)) return rc;
    return 0;
}

}  // namespace

extern "C" int dsp_internal_set_svm_lds(int dtype, int f64, int lds_bytes) {
    if (dtype == DSP_F64) return set_lds<double, double>(lds_bytes);
    return f64 ? set_lds<float, double>(lds_bytes) : set_lds<float, float>(lds_bytes);
}

extern "C" int dsp_internal_launch_svm(const SvmArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream) {
    (void)err;  // (no row of this kernel is a DSPFatal)
    if (n_wf <= 0) return 0;
    // (the planner's bounds, once more where the LDS is sized and the accumulators are counted)
    if (A->len < 1 || A->len > N_MAX || A->n_classes < 2 || A->n_classes > CLASSES_MAX || A->n_pairs != pairs(A->n_classes) || A->n_sv < 1 || !A->sv ||
        !A->sv_norm || !A->coef || !A->intercept || !A->classes || !A->label || tiles(n_wf) > 0x7fffffff || (dtype == DSP_F64 && !A->f64))
        return (int)hipErrorInvalidValue;
    const int lds = lds_bytes(A->len, A->n_pairs);
    switch (dtype) {
        case DSP_F32:
            if (A->f64)
                launch_svm<float, double>(A, n_wf, vec, lds, stream);
            else
                launch_svm<float, float>(A, n_wf, vec, lds, stream);
            break;
        case DSP_F64: launch_svm<double, double>(A, n_wf, vec, lds, stream); break;
        default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}
