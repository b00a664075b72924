// dsp_kernels.h -- what the host and the planner have to know about the kernels without seeing them: the tile constants their LDS
// footprint follows from, that footprint as constexpr functions, and the kernels' names by route.  One namespace per kernel; the kernel
// file takes its constants from here (using namespace), the planner and the host call the functions, and the CPU test programs, which
// cannot link a .hip file, see the same arithmetic.  No HIP: plain C++17.  Internal header; the public contract is include/dspeed_hip.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

// The kernels a chain can run on, in their order of precedence: a program that has the shape of several (the *_ok flags) runs on the first
// whose switch is on.  dsp_plan_route is the one place that holds this order for everything that reports a plan (kernel name, note,
// geometry); dsp_chain_execute walks the same list with the alignment of the pointers it is handed and may fall through to a later entry.
enum dsp_route {
    DSP_ROUTE_EXTREMA,  // (the one route that is no optimisation: the interpreter has no MULTI_EXTREMA, so no switch turns it off)
    DSP_ROUTE_HIST,     // (nor this one: HISTOGRAM and HISTOGRAM_STATS have no interpreter case either)
    DSP_ROUTE_THRESH,   // (nor this: MULTI_TIME_POINT_THRESH and TIME_OVER_THRESHOLD)
    DSP_ROUTE_SPECTRUM, // (nor this: PSD and FFT)
    DSP_ROUTE_SORT,     // (nor this: SORT)
    DSP_ROUTE_INTERP,   // (nor this: INTERP_UPSAMPLE)
    DSP_ROUTE_DENSE,    // (nor this: NORMALISE and DENSE)
    DSP_ROUTE_REFLECT,  // (nor this: REFLECTED_CONVOLVE)
    DSP_ROUTE_PILEUP,   // (nor this: RC_CR2 and BI_LEVEL_ZERO_CROSSING)
    DSP_ROUTE_PULSES,   // (nor this: PEAK_SNR_THRESHOLD and MULTI_A_FILTER)
    DSP_ROUTE_TAILFIT,  // (nor this: LOG_CHECK, POLY_FIT, POLY_DIFF and POLY_EXP_RMS)
    DSP_ROUTE_ALIGN,    // (nor this: INL_CORRECTION, WF_CENTROID, WF_ALIGNMENT and WF_CORRECTION)
    DSP_ROUTE_SVM,      // (nor this: SVM_PREDICT)
    DSP_ROUTE_SCALAR, DSP_ROUTE_PZ_ROWS, DSP_ROUTE_REDUCE, DSP_ROUTE_FIR_RUNS, DSP_ROUTE_CURRENT, DSP_ROUTE_FIR_F16, DSP_ROUTE_FIR_STORE,
    DSP_ROUTE_FIR_MFMA, DSP_ROUTE_ROWS, DSP_ROUTE_ENERGY_RR, DSP_ROUTE_ENERGY, DSP_ROUTE_VM
};
// a route's kernel (what rocprofv3 --kernel-trace lists)
inline constexpr const char* dsp_route_kernel_names[] = {
    "dsp_extrema_kernel",
    "dsp_hist_kernel",
    "dsp_thresh_kernel",
    "dsp_spectrum_kernel",
    "dsp_sort_kernel",
    "dsp_interp_kernel",
    "dsp_dense_kernel",
    "dsp_reflect_kernel",
    "dsp_pileup_kernel",
    "dsp_pulses_kernel",
    "dsp_tailfit_kernel",
    "dsp_align_kernel",
    "dsp_svm_kernel",
    "dsp_scalar_kernel",    "dsp_pz_rows_kernel",  "dsp_reduce_kernel", "dsp_fir_runs_kernel",  "dsp_current_kernel", "dsp_fir_f16_kernel",
    "dsp_fir_store_kernel", "dsp_fir_mfma_kernel", "dsp_rows_kernel",   "dsp_energy_rr_kernel", "dsp_energy_kernel",  "dsp_vm_kernel<float>"};
static_assert(sizeof dsp_route_kernel_names / sizeof dsp_route_kernel_names[0] == DSP_ROUTE_VM + 1, "a name per route");

namespace dsp_hist {  // dsp_hist.hip: a uint32 counter per bin (rounded up to whole rounds of 64 lanes) for each of a workgroup's four wavefronts
constexpr int WAVES = 4;
constexpr int lds_bytes(int m) { return WAVES * ((m + 63) & ~63) * 4; }
}  // namespace dsp_hist

namespace dsp_spectrum {  // dsp_spectrum.hip: a row's transform as (re, im) pairs of the loop's type in LDS
// complex points of the transform of a row of n samples: n / 2 for a power of two (the real row packed in pairs; 1 for n <= 2), else
// Bluestein's padded length, the power of two >= 2 n - 1
constexpr bool pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }
constexpr int points(int n) {
    if (pow2(n)) return n >= 2 ? n / 2 : 1;
    int m = 1;
    while (m < 2 * n - 1) m *= 2;
    return m;
}
constexpr int row_bytes(int n, int esz) { return points(n) * 2 * esz; }
// the geometry: rows whose transform fills at most this much LDS get a wavefront each, four to a workgroup (32 KiB); longer ones a
// workgroup of 256 (up to 64 KiB), with 16 bytes behind the transform for the word its wavefronts agree through
constexpr int WAVE_ROW_BYTES = 8 * 1024;
constexpr bool wide(int n, int esz) { return row_bytes(n, esz) > WAVE_ROW_BYTES; }
constexpr int lds_bytes(int n, int esz) { return wide(n, esz) ? row_bytes(n, esz) + 16 : 4 * row_bytes(n, esz); }
}  // namespace dsp_spectrum

namespace dsp_sort {  // dsp_sort.hip: a row as order-preserving unsigned keys in LDS, sorted by a bitonic network over the padded length P
// ---- keys.  The bits of a sample map to an unsigned key whose integer order is the samples' order: all bits of a negative value flipped,
// the sign bit of any other set.  -0.0 lands just below +0.0, -inf .. +inf fill [KEY_NEG_INF, KEY_POS_INF], and every NaN lies outside
// that range on one side or the other: one unsigned comparison finds it.
constexpr uint32_t key_of(uint32_t bits) { return bits & 0x80000000u ? ~bits : bits | 0x80000000u; }
constexpr uint64_t key_of(uint64_t bits) { return bits & 0x8000000000000000ull ? ~bits : bits | 0x8000000000000000ull; }
constexpr uint32_t bits_of(uint32_t key) { return key & 0x80000000u ? key & 0x7fffffffu : ~key; }
constexpr uint64_t bits_of(uint64_t key) { return key & 0x8000000000000000ull ? key & 0x7fffffffffffffffull : ~key; }
constexpr uint32_t KEY_NEG_INF32 = 0x007fffffu, KEY_POS_INF32 = 0xff800000u;
constexpr uint64_t KEY_NEG_INF64 = 0x000fffffffffffffull, KEY_POS_INF64 = 0xfff0000000000000ull;
constexpr bool key_is_nan(uint32_t key) { return (uint32_t)(key - KEY_NEG_INF32) > KEY_POS_INF32 - KEY_NEG_INF32; }
constexpr bool key_is_nan(uint64_t key) { return (uint64_t)(key - KEY_NEG_INF64) > KEY_POS_INF64 - KEY_NEG_INF64; }

// ---- geometry.  A lane holds CHUNK neighbouring keys in registers, a wavefront a TILE of 64 chunks.  A row of n samples is padded with
// +inf keys to P = padded(n): the power of two >= n, and at least a chunk.  Rows of P <= NARROW_MAX get a wavefront each, four rows to a
// workgroup; longer rows a workgroup of 256, with 16 bytes behind the keys for the word its wavefronts agree on "a NaN" through.
constexpr int CHUNK = 8, TILE = 64 * CHUNK;
constexpr int NARROW_MAX = 2048;
constexpr int padded(int n) {
    int p = CHUNK;
    while (p < n) p *= 2;
    return p;
}
constexpr bool wide(int n) { return padded(n) > NARROW_MAX; }
constexpr int lds_bytes(int n, int esz) { return wide(n) ? padded(n) * esz + 16 : 4 * padded(n) * esz; }

// ---- schedule.  Stage k = 2, 4 .. P merges bitonic runs of k keys with the steps j = k / 2, k / 4 .. 1; step (k, j) compares key i with
// key i ^ j and leaves the smaller at the lower index where bit k of i is clear (the run ascends), the larger where it is set.  The last
// stage's k is P, which no index has: everything ascends.  A step's stride says where its two keys meet: inside a lane's chunk, in two
// lanes of a wavefront's tile, or only in LDS.
struct Step {
    int k, j;
};
constexpr int log2_of(int p) {
    int l = 0;
    while ((1 << l) < p) ++l;
    return l;
}
constexpr int steps(int P) { return log2_of(P) * (log2_of(P) + 1) / 2; }
constexpr Step step(int P, int s) {  // the s-th of steps(P), in the order they run
    (void)P;
    int stage = 1;
    while (s >= stage) s -= stage, ++stage;
    return {1 << stage, 1 << (stage - 1 - s)};
}
constexpr int partner(int i, int j) { return i ^ j; }
constexpr bool ascends(int i, int k) { return (i & k) == 0; }
constexpr bool keeps_min(int i, int k, int j) { return ((i & j) == 0) == ascends(i, k); }
enum Kind { REGISTER, CROSS_LANE, LDS };
constexpr Kind kind(int j) { return j < CHUNK ? REGISTER : j < TILE ? CROSS_LANE : LDS; }
// LDS passes over a row behind the staging: one that runs stages 2 .. min(P, TILE) on a tile in registers, then per longer stage one per
// LDS step and one for the steps below TILE
constexpr int lds_passes(int P) {
    int passes = 1;
    for (int k = 2 * TILE; k <= P; k *= 2) passes += log2_of(k / TILE) + 1;
    return passes;
}
}  // namespace dsp_sort

namespace dsp_interp {  // dsp_interp.hip: interpolating_upsampler (upsampler.py:52-216), a row of n samples in LDS resampled to m outputs
// ---- index rules.  The reference walks the INPUT samples and fills intervals of outputs whose bounds are float64 expressions of
// u = m / n: one division, then one multiply with one rounding per bound -- not the rational ceil(m i / n), from which they differ (at
// i = 7 for (n, m) = (14, 58)).  The kernel walks the OUTPUTS, so the rules are inverted here: a candidate floor(o / u), corrected by
// evaluating the reference's own bound expression.  bound(mode, u, i) is the first output that input sample i does NOT fill:
//   'n' ceil(u (i + 0.5))     'f' 'l' 'h' ceil(u (i + 1))     'c' floor(u i) + 1     's' ceil(u (i + 1)) + 1
// ('s' writes each segment from its upper bound down to ceil(u i) inclusive, lower segments later: an output that is a segment bound
// keeps the value of the lower segment, evaluated at t0 >= 1.)
constexpr int64_t ceil_of(double x) {  // x >= 0, below 2^62
    const int64_t k = (int64_t)x;
    return k + ((double)k < x ? 1 : 0);
}
constexpr double ratio(int n, int64_t m) { return (double)m / (double)n; }
constexpr int64_t bound(int mode, double u, int i) {
    return mode == 'n' ? ceil_of(u * ((double)i + 0.5)) : mode == 'c' ? (int64_t)(u * (double)i) + 1 : ceil_of(u * (double)(i + 1)) + (mode == 's' ? 1 : 0);
}
enum Kind { VALUE, ZERO, TAIL, NONE };  // a segment's value / one of 'i's zeros / 'n' and 'c': w_in[n - 1] behind the last bound / left NaN
struct Map {
    int seg;  // the input sample (n f c i), the lower sample of the segment (l h s); TAIL: n - 1
    Kind kind;
};
// the smallest i in [from, n) with o < bound(i), n if there is none; `from` is at most that i (bounds do not decrease with i)
constexpr int advance(int mode, int n, double u, int64_t o, int from) {
    int i = from;
    while (i < n && !(o < bound(mode, u, i))) ++i;
    return i;
}
constexpr int locate(int mode, int n, double u, int64_t o) {
    const double q = (double)o / u;
    int i = q < (double)(n - 1) ? (int)q : n - 1;
    while (i > 0 && o < bound(mode, u, i - 1)) --i;
    return advance(mode, n, u, o, i);
}
// what output o is made of, given i = locate(...) or advance(...) of it
constexpr Map map_of(int mode, int n, int64_t m, int64_t o, int i) {
    if (mode == 'i') {
        const int64_t r = m / n;
        return {(int)(o / r), o % r ? ZERO : VALUE};
    }
    if (mode == 'h' || mode == 's') return {i < n - 2 ? i : n - 2, n < 2 ? NONE : VALUE};  // ('h': the last segment extrapolates; 's' at n == 1: NaNs)
    if (i < n) return {i, VALUE};
    return {n - 1, mode == 'n' || mode == 'c' ? TAIL : NONE};
}
constexpr Map map(int mode, int n, int64_t m, int64_t o) { return map_of(mode, n, m, o, mode == 'i' ? 0 : locate(mode, n, ratio(n, m), o)); }
constexpr bool mode_ok(int mode) { return mode == 'i' || mode == 'n' || mode == 'f' || mode == 'c' || mode == 'l' || mode == 'h' || mode == 's'; }

// ---- the spline's sweeps.  The forward coefficient w2[i] = -0.5 / (0.5 w2[i - 1] + 2) is data independent and stationary in float64 from
// i = STATIONARY on; both recurrences contract by 0.268 a step, so WARM samples of warm-up put a perturbation of 3e-28 ahead of the same
// operations (pickoff_spline's argument, dsp_vm.hip).
constexpr int WARM = 48, STATIONARY = 15;
constexpr double W2_FIX = -0.2679491924311227;
constexpr double forward_coef(int i) {  // w2[i] of the forward sweep, 1 <= i <= n - 2 (0 outside)
    if (i >= STATIONARY) return W2_FIX;
    double w = 0.0;
    for (int k = 1; k <= i; ++k) w = -0.5 / (0.5 * w + 2.0);
    return w;
}

// ---- geometry.  The row lives in LDS in the loop's type, the spline's second derivatives as float64 behind it.  Rows of up to
// WAVE_ROW_BYTES get a wavefront each, four to a workgroup (no barrier); longer ones a workgroup of 256, with 16 bytes behind the row for
// the word its wavefronts agree on "a NaN" / "an infinity" through.
constexpr int WAVE_ROW_BYTES = 8 * 1024, LDS_MAX = 64 * 1024;
constexpr int w2_offset(int n, int esz) { return (n * esz + 15) / 16 * 16; }  // bytes from the row to the second derivatives
constexpr int row_bytes(int mode, int n, int esz) { return w2_offset(n, esz) + (mode == 's' ? (n * 8 + 15) / 16 * 16 : 0); }
constexpr bool wide(int mode, int n, int esz) { return row_bytes(mode, n, esz) > WAVE_ROW_BYTES; }
constexpr int lds_bytes(int mode, int n, int esz) { return wide(mode, n, esz) ? row_bytes(mode, n, esz) + 16 : 4 * row_bytes(mode, n, esz); }
constexpr int SPLINE_F32_MAX = 5456, SPLINE_F64_MAX = 4096;  // (with LDS_MAX / esz for the other modes: DSP_INTERP_*_MAX of dsp_program.h)
constexpr int max_len(int mode, int esz) { return mode == 's' ? (esz == 8 ? SPLINE_F64_MAX : SPLINE_F32_MAX) : LDS_MAX / esz; }
static_assert(row_bytes('s', SPLINE_F32_MAX, 4) <= LDS_MAX && row_bytes('s', SPLINE_F32_MAX + 16, 4) > LDS_MAX, "the longest float32 spline row fills the LDS");
static_assert(row_bytes('s', SPLINE_F64_MAX, 8) == LDS_MAX && row_bytes('l', max_len('l', 4), 4) == LDS_MAX, "and the others");
}  // namespace dsp_interp

namespace dsp_dense {  // dsp_dense.hip: the neural-network layers of ml.py, rows x an (n, m) weight matrix on the matrix cores
// ---- geometry.  A workgroup of WAVES wavefronts takes TILE_ROWS rows and all m outputs; a wavefront WAVE_ROWS rows x m, m in blocks of BLOCK
// columns, an accumulator tile of v_mfma_*_16x16x4 per block.  Rows and weights pass through LDS in chunks of 256 bytes a row along n:
//   x  [TILE_ROWS][x_pitch]    the rows' chunk, zero beyond n and in the rows beyond the batch
//   w  [chunk][w_pitch(m)]     the weights' chunk, zero beyond n and in the columns beyond m (0 x garbage may be NaN)
// Pitches: the lanes of an operand read differ in row (l & 15, x) or column (l & 15, w) and in k (l >> 4); the pads put the four k of a
// read into different banks.
constexpr int WAVES = 4, WAVE_ROWS = 16, TILE_ROWS = WAVES * WAVE_ROWS, BLOCK = 16, DEPTH = 4;  // (DEPTH: the k of one instruction)
constexpr int N_MAX = 16384, M_MAX = 256, BLOCKS_MAX = M_MAX / BLOCK;
constexpr int chunk(int esz) { return 256 / esz; }
constexpr int x_pitch(int esz) { return chunk(esz) + 16 / esz; }
constexpr int blocks(int m) { return (m + BLOCK - 1) / BLOCK; }
constexpr int w_pitch(int m) { return blocks(m) * BLOCK + (blocks(m) % 2 == 0 ? BLOCK : 0); }
constexpr int lds_bytes(int m, int esz) { return m < 1 ? 0 : (chunk(esz) * w_pitch(m) + TILE_ROWS * x_pitch(esz)) * esz; }
// the kernel is built for 1, 4 or BLOCKS_MAX column blocks a wavefront: the smallest that holds m
constexpr int built_blocks(int m) { return blocks(m) <= 1 ? 1 : blocks(m) <= 4 ? 4 : BLOCKS_MAX; }
constexpr int64_t tiles(int64_t n_wf) { return (n_wf + TILE_ROWS - 1) / TILE_ROWS; }
static_assert(lds_bytes(M_MAX, 4) == 87040 && lds_bytes(M_MAX, 8) == 87040 && lds_bytes(1, 4) < 64 * 1024, "LDS of the widest layer: raised past 64 KiB (dsp_internal_set_dense_lds)");
}  // namespace dsp_dense

namespace dsp_svm {  // dsp_svm.hip: svm_predict (svm.py:13-71), an RBF or linear one-vs-one SVC: two chained float64 products on the matrix cores
// ---- geometry.  dsp_dense's tile of rows: a workgroup of WAVES wavefronts takes TILE_ROWS rows, a wavefront WAVE_ROWS.  The support vectors
// come SV_BLOCK at a time, SV_TILES accumulator tiles of v_mfma_f64_16x16x4 a wavefront, transposed: G^T = SV . X^T, so that a tile's
// register r (support vectors 4 r .. 4 r + 3 of the tile, a row per lane & 15) is, once K is formed from it, the B operand of
// DEC^T += D^T . K^T as it stands.  DEC^T lives in pair_blocks(P) accumulator tiles of BLOCK pairs across all support-vector blocks.
//   x   [TILE_ROWS][x_pitch(n)]   the rows as float64: whole (n <= RESIDENT_MAX, staged once) or a chunk of KC samples, staged again per block
//   sv  [SV_BLOCK][SV_PITCH]      the support vectors' chunk, zero beyond n and beyond n_sv
//   dec [TILE_ROWS][dec_pitch(P)] behind the last block, over the same bytes: a row's decisions, for its vote
// Pitches: dsp_dense's -- the lanes of an operand read differ in row (l & 15) and in k (l >> 4).
using dsp_dense::BLOCK;
using dsp_dense::DEPTH;
using dsp_dense::N_MAX;
using dsp_dense::TILE_ROWS;
using dsp_dense::tiles;
using dsp_dense::WAVE_ROWS;
using dsp_dense::WAVES;
constexpr int CLASSES_MAX = 23, P_MAX = 256, PAIR_BLOCKS_MAX = P_MAX / BLOCK;  // (DSP_SVM_CLASSES_MAX of dsp_program.h)
constexpr int KC = 32, SV_TILES = 4, SV_BLOCK = SV_TILES * BLOCK, SV_PITCH = KC + 2;
constexpr int RESIDENT_MAX = 256;
constexpr int pairs(int k) { return k * (k - 1) / 2; }
constexpr int pair(int i, int j, int k) { return i * (2 * k - i - 1) / 2 + (j - i - 1); }  // (i < j) in the order (0,1), (0,2) .. (k-2,k-1)
constexpr bool resident(int n) { return n <= RESIDENT_MAX; }
constexpr int x_cols(int n) { return resident(n) ? (n + KC - 1) / KC * KC : KC; }
constexpr int x_pitch(int n) { return x_cols(n) + 2; }
constexpr int pair_blocks(int P) { return (P + BLOCK - 1) / BLOCK; }
// the kernel is built for 1, 4 or PAIR_BLOCKS_MAX blocks of pairs a wavefront: the smallest that holds P
constexpr int built_blocks(int P) { return pair_blocks(P) <= 1 ? 1 : pair_blocks(P) <= 4 ? 4 : PAIR_BLOCKS_MAX; }
constexpr int dec_pitch(int P) { return pair_blocks(P) * BLOCK + 1; }
constexpr int stage_bytes(int n) { return (TILE_ROWS * x_pitch(n) + SV_BLOCK * SV_PITCH) * 8; }
constexpr int vote_bytes(int P) { return TILE_ROWS * dec_pitch(P) * 8; }
constexpr int lds_bytes(int n, int P) { return stage_bytes(n) > vote_bytes(P) ? stage_bytes(n) : vote_bytes(P); }
// what the kernels' dynamic-LDS limit is raised to, once, whatever a chain needs: chains of one row type share a kernel, and a smaller
// value set for a later chain would undercut an earlier one's launches
constexpr int LDS_MAX = lds_bytes(RESIDENT_MAX, P_MAX);
static_assert(LDS_MAX >= lds_bytes(N_MAX, P_MAX) && LDS_MAX >= lds_bytes(RESIDENT_MAX, 1), "the largest of both areas");
static_assert(pairs(CLASSES_MAX) <= P_MAX && pairs(CLASSES_MAX + 1) > P_MAX && pair(0, 1, 4) == 0 && pair(1, 2, 4) == 3 && pair(2, 3, 4) == 5, "the pairs of the most classes fill the accumulators");
static_assert(lds_bytes(RESIDENT_MAX, P_MAX) == 149504 && lds_bytes(N_MAX, 1) == 34816 && lds_bytes(N_MAX, P_MAX) == 131584, "LDS of the longest resident rows: raised past 64 KiB (dsp_internal_set_svm_lds)");
}  // namespace dsp_svm

namespace dsp_reflect {  // dsp_reflect.hip: reflected_convolve_wf (convolutions.py:122-182), a FIR of m taps over a row of n samples with mirrored edges
// ---- the rule.  np.convolve(np.pad(w, int(m/2) + 1, "reflect"), kernel, "same") cut back to n samples is, for 1 <= m <= n,
//   out[i] = sum_k kernel[k] * w[reflect(i + centre(m) - k, n)]
// the kernel flipped (a convolution), its centre at (m - 1) / 2 for even m too, the edge sample not repeated ("reflect", not "symmetric").
// One reflection suffices because m <= n.
constexpr int centre(int m) { return (m - 1) / 2; }
constexpr int left(int m) { return m / 2; }         // mirrored samples ahead of the row: output 0 reaches centre(m) - (m - 1) = -left(m)
constexpr int right(int m) { return (m - 1) / 2; }  // and behind it: output n - 1 reaches n - 1 + centre(m)
constexpr int reflect(int t, int n) { return t < 0 ? -t : t > n - 1 ? 2 * (n - 1) - t : t; }
// ---- the staged row.  staged(n, m) samples E[j] = w[source(j, n, m)], the margins materialised beside the row, so that
//   out[i] = sum_k kernel[k] * E[i + m - 1 - k]
// needs no branch.  A lane makes vec(esz) consecutive outputs and reads its samples 16 bytes at a time, V taps a step from tap 0 on: the
// staged row starts pad(m, esz) samples into its LDS, so that these reads are whole vectors -- output i, taps k0 .. k0 + V - 1 (k0 a
// multiple of V) read the vector at i + m + pad - k0 - V and, for its later outputs, those above; the last step of a kernel whose length
// is no multiple of V starts at 0 and uses its upper m % V samples only.  elems(): the samples of LDS a row takes, the run of the last lane
// included (what it reads past the staged row feeds outputs past the row, which are not stored).
constexpr int staged(int n, int m) { return n + m - 1; }
constexpr int source(int j, int n, int m) { return reflect(j - left(m), n); }
constexpr int vec(int esz) { return 16 / esz; }
constexpr int round_up(int x, int v) { return (x + v - 1) / v * v; }
constexpr int pad(int m, int esz) { return round_up(m, vec(esz)) - m; }
constexpr int elems(int n, int m, int esz) { return round_up(n, vec(esz)) + round_up(m, vec(esz)); }
// ---- geometry and limits.  The staged row lives in 64 KiB of LDS: F32_MAX / F64_MAX staged samples (DSP_REFLECT_*_MAX of dsp_program.h);
// the alignment above adds at most 28 bytes.  Rows that fill at most WAVE_ROW_BYTES staged get a wavefront each, four to a workgroup (no
// barrier); longer ones a workgroup of 256, with 16 bytes behind the row for the word its wavefronts agree on "a NaN" through.
constexpr int WAVE_ROW_BYTES = 8 * 1024, LDS_MAX = 64 * 1024;
constexpr int F32_MAX = LDS_MAX / 4, F64_MAX = LDS_MAX / 8;
constexpr int max_staged(int esz) { return esz == 8 ? F64_MAX : F32_MAX; }
constexpr bool fits(int n, int m, int esz) { return (int64_t)n + m - 1 <= max_staged(esz); }
constexpr int row_bytes(int n, int m, int esz) { return elems(n, m, esz) * esz; }
constexpr bool wide(int n, int m, int esz) { return staged(n, m) * esz > WAVE_ROW_BYTES; }
constexpr int lds_bytes(int n, int m, int esz) { return wide(n, m, esz) ? row_bytes(n, m, esz) + 16 : 4 * row_bytes(n, m, esz); }
static_assert(left(1) == 0 && right(1) == 0 && left(4) == 2 && right(4) == 1 && left(4) + right(4) + 1 == 4, "the margins of a kernel");
static_assert(lds_bytes(F32_MAX, 1, 4) == LDS_MAX + 16 + 16 && lds_bytes(F64_MAX - 1, 2, 8) <= LDS_MAX + 16 + 16, "the longest rows: raised past 64 KiB (dsp_internal_set_reflect_lds)");
}  // namespace dsp_reflect

namespace dsp_pileup {  // dsp_pileup.hip: rc_cr2 and bi_level_zero_crossing_time_points, one waveform per lane
// The 64 rows of a wavefront pass through one LDS tile of TS samples each: written along the rows, read along the columns -- lane l walks
// row l of the tile --, and a filtered row goes back through the same tile.  With a pitch of TS + 1 elements the lanes of a column read hit
// different banks in both loops (float32: bank (65 l) % 32 = l % 32 within a half of the wavefront; float64: dwords 130 l, 130 l + 1).
constexpr int ROWS = 64, TS = 64, PITCH = TS + 1;
constexpr int lds_bytes(int esz) { return ROWS * PITCH * esz; }
constexpr int64_t tiles(int64_t n_wf) { return (n_wf + ROWS - 1) / ROWS; }
constexpr int MIN_FILTER_LEN = 4;  // rc_cr2.py:51-54: more than 3 samples
static_assert(lds_bytes(8) <= 64 * 1024, "a static LDS array");
}  // namespace dsp_pileup

namespace dsp_tailfit {  // dsp_tailfit.hip: log_check, poly_fit, poly_diff and poly_exp_rms, one waveform per lane
// The rows pass through the pile-up kernel's tile (dsp_lane_tiles.h), twice where the residuals follow the fit.  Beside it lies the table of
// the powers of a tile's sample indices: float64(i**j) for the TS samples of the tile and j < POLY_MAX, which a lane forms for one sample
// and all lanes read, every lane the same entry at a time (a broadcast).
using dsp_pileup::PITCH;
using dsp_pileup::ROWS;
using dsp_pileup::tiles;
using dsp_pileup::TS;
constexpr int POLY_MAX = 8;  // DSP_POLY_MAX (dsp_program.h)
constexpr int lds_bytes(int esz) { return dsp_pileup::lds_bytes(esz) + TS * POLY_MAX * 8; }
static_assert(lds_bytes(8) <= 64 * 1024, "static LDS arrays");
}  // namespace dsp_tailfit

namespace dsp_pulses {  // dsp_pulses.hip: peak_snr_threshold (peak_snr_threshold.py:19-71) and multi_a_filter (multi_a_filter.py:20-57)
// ---- the rule of a candidate, shared by the kernel, the planner and tests/pulse_window.cpp.  A candidate idx of a row of n samples, the
// window half width `width` >= 0: c = int(idx) (towards zero), the minimum is looked for over j in [a, b) from min_index = a,
//   a = max(c - width, 0),  b = min(c + width, n - 1)
// -- b itself is never looked at, so neither c + width nor, under the clamp, the row's last sample; an empty window leaves a.  dropped():
// the candidates no sample is read for -- a NaN (the reference skips it), and where the reference defines nothing: an infinite one, and one
// whose int() lies outside [0, n).  The test is made on the value, before any conversion: (-1, n) is what truncates into [0, n - 1].
struct Window {
    int c, a, b;
};
constexpr bool dropped(double idx, int n) { return !(idx > -1.0 && idx < (double)n); }  // (a NaN fails both comparisons)
constexpr Window window(double idx, int n, int width) {
    const int c = (int)idx;  // (not dropped: -1 < idx < n)
    const int64_t lo = (int64_t)c - width, hi = (int64_t)c + width;
    return {c, (int)(lo < 0 ? 0 : lo), (int)(hi >= n ? n - 1 : hi)};
}
// the width as the kernel takes it: int(width_in), and at most n -- beyond that both ends are clamped whatever the candidate
constexpr int clamped_width(double width_in, int n) { return width_in >= (double)n ? n : (int)width_in; }
static_assert(window(5.9, 10, 2).c == 5 && window(5.9, 10, 2).a == 3 && window(5.9, 10, 2).b == 7 && window(8.0, 10, 3).b == 9 && window(-0.5, 10, 3).c == 0, "the window");
static_assert(dropped(-1.0, 10) && dropped(10.0, 10) && !dropped(-0.999, 10) && !dropped(9.5, 10) && dropped(0.0, 0), "the dropped candidates");
}  // namespace dsp_pulses

namespace dsp_current {  // dsp_current.hip
constexpr int CB = 16;   // samples per block (= per checkpoint)
constexpr int lds_bytes(int ma_len) { return (ma_len / CB + 1) * CB * 64 * 4; }
}  // namespace dsp_current

namespace dsp_fir_mfma {  // dsp_fir_mfma.hip: the amax kernel and the kept-output ("store") kernel
constexpr int BM = 64, BN = 320, APITCH = 36;
constexpr int TB = BN + 4;
constexpr int lds_bytes(int kend) { return (((BN + kend + 3) & ~3) + 2 * BM * APITCH + BM * 4 * 2) * 4; }
constexpr int store_lds_bytes(int kend) { return (((TB + kend + 3) & ~3) + 2 * BM * APITCH) * 4; }
}  // namespace dsp_fir_mfma

// A/B builds of the float16 FIR: build.py hands its defines to every unit, so the host sizes what the kernel was built for
#ifndef F16_BK
#define F16_BK 64
#endif
#ifndef F16_BM
#define F16_BM 64
#endif
namespace dsp_fir_f16 {  // dsp_fir_f16.hip
constexpr int BM = F16_BM, BK = F16_BK;  // BM 64: 8 wavefronts (2 x 4); BM 32: 4 wavefronts, two workgroups per CU
// LDS reads are ds_read_b128: four fixed groups of 16 lanes per instruction, 64 banks -- a group is conflict-free when its 16 addresses fall
// into 16 different 16-byte slots of the 256-byte bank line (MI355X_MICROARCH.md, LDS).
constexpr int APITCH = BK + 16;  // halfs per A row: 10 (BK 64) / 18 (BK 128) slots, = 2 modulo 16: lane (row j, k-block h) sits in slot 10 j + h, no two alike in a group
constexpr int TB = 336;          // zero margin below tap 0: window index TB + k - column - e - shift is never negative
constexpr int TWIN = TB + BK;    // taps a stage's fragments can reach
// a tap copy in LDS: a multiple of 256 bytes, so that a copy's slot is its own offset only; copy r starts tap_slot[e][r] slots in -- for
// every alignment e of the window a table that puts the 16 lanes of every group (eight columns x two k-blocks, five copies apart at most
// identical addresses, which broadcast) into 16 different slots (found by search, tools/fir_f16_banks.py; the plain pitch had 51 % of the
// LDS-array cycles as conflicts)
constexpr int TPITCH = ((TWIN + 8 + 15 * 8 + 127) / 128) * 128;
// halfs of the tap image of one kernel: 16 copies of TZ = the longest K window rounded up to a stage + the window the last stage reaches +
// the margin the shifted copies reach into, then the inverse scale (one float, kept 16-byte aligned)
constexpr int tz(int kend) { return ((kend + 8 + BK - 1) / BK) * BK + TWIN + 16; }
constexpr size_t taps_bytes(int kend) { return (size_t)16 * tz(kend) * 2 + 16; }
constexpr int lds_bytes() { return (2 * 2 * BM * APITCH + 2 * 16 * TPITCH) * 2 + (BM * 4 * 2 + BM) * 4; }
}  // namespace dsp_fir_f16

namespace dsp_fir_runs {    // dsp_fir_runs.hip
constexpr int STEP = 512;  // samples per step: 8 per lane
constexpr int lds_bytes(int m) {
    const int mp = (m + 63) & ~63;
    return (4 * (mp + mp / 8 + STEP + STEP / 8) + 64) * (int)sizeof(double);  // (+ the round of the window's copy that reads past the last window)
}
}  // namespace dsp_fir_runs

namespace dsp_rows {    // dsp_rows.hip
constexpr int RB = 8;  // samples per block (= per barrier)
constexpr int ring_entries(int maxlag) { return ((maxlag + RB + RB - 1) / RB) * RB; }  // R > largest lag + 7, a whole number of blocks
constexpr int lds_bytes(int R) { return (R + RB) * 64 * 4; }                           // the history ring and the block in flight, 64 lanes
}  // namespace dsp_rows

// The register-resident energy kernel's LDS region of one wavefront (dsp_energy.hip), in float32 elements, for C samples per lane: `guard`
// zeros below the image (lagged reads before sample 0; an odd lag's pairs start one element lower: covered), the image of 64 C elements at
// slot_off (16-byte aligned), `tail` elements above it, a side array of side_pitch (odd) elements per lane for the (C - 2) / 8 + 1 group
// sums, a capture buffer of 2 x 16.  The guard holds 2 C + 8 elements for the windows that straddle sample 0 and at least C + 72 for
// the ones wholly below it (lag_window_start): 1024 and 2048 samples get 46 and 30 elements more than 2 C + 8 for that.
namespace dsp_energy_rr {
struct Layout {
    int guard, slot_off, tail, side_pitch, elems;
};
constexpr int WINDOW_SPAN_EXTRA = 8;  // a lane reads C + 2 elements from its window's aligned start (an odd lag's extra pair, the tail's), the 4-point re-run up to C + 7
constexpr Layout layout(int C) {
    const int guard = 2 * C + 8 > C + 72 ? 2 * C + 8 : C + 72, slot_off = (guard + 3) / 4 * 4, tail = 16, ng1 = (C - 2) / 8 + 1;
    const int side_pitch = ng1 <= 9 ? 9 : (ng1 | 1);  // (9 for up to 4096 samples, 17 for 8192)
    return {guard, slot_off, tail, side_pitch, (slot_off + 64 * C + tail + 64 * side_pitch + 2 * 16 + 3) / 4 * 4};
}
// Where lane `lane` starts to read the stream that lags by `lag` samples, as an element of the image (sample i at element i; negative:
// the guard), always even.  Its window is samples lane C - lag .. lane C - lag + C - 1, read as aligned pairs from `natural` = that start
// minus the lag's parity.  A window that holds a sample >= 0 keeps its natural start.  One wholly below sample 0 reads zeros wherever it
// reads them, and if all such lanes read one address that address shares a bank pair with one of the reading lanes in every access.  So
// each reads at the guard address that equals its natural one modulo 64 elements (the 64 banks of an 8-byte access of 32 lanes): natural
// plus the smallest multiple of 64, of either sign, that brings it to -guard or above.  That is below -guard + 64, so the C +
// WINDOW_SPAN_EXTRA elements from it end at or below element 0 when guard >= C + 72.  Natural starts of the 32 lanes of a half are C
// apart, C / 2 is odd: 32 different pairs of banks, redirected or not.
constexpr int lag_window_start(int C, int guard, int lane, int lag) {
    const int natural = lane * C - lag - (lag & 1);
    if (lane * C - lag + C > 0) return natural;
    const int d = -guard - natural;  // > 0: natural lies that far below the guard, up by the next multiple of 64; < 0: that far inside or above it, down by whole 64s
    return natural + (d >= 0 ? (d + 63) / 64 * 64 : -((-d) / 64 * 64));
}
}  // namespace dsp_energy_rr
