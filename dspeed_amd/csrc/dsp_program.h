// dsp_program.h -- everything that crosses from the planner and the host (dsp_plan.cpp, dsp_host.cpp) to a kernel by value: the device-side
// program of the waveform VM (dsp_vm.hip) and the argument block of every specialised kernel, each defined here and nowhere else.  No HIP:
// the planner fills these on the CPU.  Internal: the public contract is include/dspeed_hip.h.
#pragma once
#include <stdint.h>

#include "../../include/dspeed_hip.h"

#define DSP_WAVE 64
#define DSP_FC 40 /* host-precomputed float64 constants per op */
#define DSP_OP_INTERNAL_NOP 101  /* host-made: a BL_SUBTRACT that the LOAD in front of it does while it writes the samples (DevOp ic[0] of the LOAD) */
#define DSP_OP_INTERNAL_STORES 102 /* host-made: a run of STORE_SCALAR ops as one op -- dst = count (<= DSP_IC), ic[j] = binding | register << 16: lane j stores */
#define DSP_OP_INTERNAL_ZERO 100 /* host-inserted: clear slot dst's whole LDS region (guard, chunks, pads, tail) before its first use */
#define DSP_SCRATCH_ELEMS 128
#define DSP_IC 12 /* host-precomputed integer constants per op */

// One waveform variable living in LDS.  Lane j of the wavefront owns samples [j*C, (j+1)*C) ("chunk");
// chunk j starts at element off + j*pitch with pitch = C+1 (odd) so that "every lane reads offset t of
// its chunk" hits 64 different banks.  Samples >= len up to 64*C are kept finite (zero-filled at load).
// FIR inputs are laid out without the pad (padw = 0, pitch = C: sample i at element off + i) so that a lane's
// window of consecutive samples is addressed with immediate offsets.
struct DevSlot {
    int32_t off;   // element offset inside the wavefront's LDS region
    int32_t len;   // logical number of samples
    int32_t C;     // samples per lane, multiple of 8
    int32_t pitch; // C + 1
    float invC;    // 1/C for index -> (lane, offset) splits
    int32_t padw;  // pitch - C: 1 (chunk pad) or 0 (linear)
    // elements that are guaranteed to read 0 below sample 0 (the guard) and above sample len - 1 (the tail; 0 unless len == 64 * C:
    // a partial last chunk is only "finite"): a FIR window may reach that far outside the waveform without bounds checks
    int32_t zero_below, zero_above;
};

struct DevIO {
    int32_t kind, dtype, len, offset;
    int64_t row_stride;
    int32_t vec_ok; // row base, stride and offset keep 16-byte alignment -> wide loads/stores
    int32_t pad_;
};

#define DSP_MEMBER_ALL 15
struct DevOp {
    int32_t opcode, dst, src, io;
    int32_t ip[4];
    dsp_scalar_arg sp[4];
    int32_t ic[DSP_IC];
    int32_t member;  // DevProgram.team > 1: which wavefront of a row's team runs the op (0 .. team - 1; DSP_MEMBER_ALL: every member)
    int32_t prio;    // the wave priority the interpreter runs the op at: 0 .. 3 over the op list (the planner's division, not one per op and row)
    double fc[DSP_FC];
};

struct DevProgram {
    int32_t n_ops, n_slots, n_io, n_sregs;
    int32_t lds_elems_per_wave; // waveform slots + scalar registers, in elements of the compute type
    int32_t sreg_off;           // element offset of the scalar register file
    int32_t waves_per_block;
    int32_t scratch_off;        // element offset of DSP_SCRATCH_ELEMS elements any op may use while it runs (16-byte aligned)
    // 2, 3: a TEAM of wavefronts per row -- a program that loads one waveform and then only reads it (reductions, walks, pick-offs of long
    // waveforms, whose image leaves LDS for one wavefront per SIMD) splits into groups of ops that share no register; each member runs
    // its groups on the shared image (DevOp.member).  1: a wavefront per row
    int32_t team;
    int32_t pad_;
    // per-op cycle counters (dsp_chain_profile): n_ops + 1 device words, the last counts the waveforms sampled; null = off
    unsigned long long* prof;
    DevSlot slots[DSP_MAX_SLOTS];
    DevIO io[DSP_MAX_IO];
    DevOp ops[DSP_MAX_OPS + DSP_MAX_SLOTS]; // + one region-clearing op per slot that shares LDS (DSP_OP_INTERNAL_ZERO)
};

struct IoPtrs {
    void* p[DSP_MAX_IO];
};

// device error word layout: err[0] = DSP_E_* code (0 = none), err[1..2] = row (lo, hi); behind the diagnostic sums, word DSP_ERR_TABLE_WORD:
// the aligner's "the table holds a NaN" (dsp_align.hip), cleared and written by every launch that has a table
#define DSP_ERR_TABLE_WORD 16
#define DSP_ERR_WORDS 20 /* 4 error words + 6 x 64-bit diagnostic phase-cycle sums */

// arguments of the lane-per-waveform fit kernel (dsp_fit.hip), filled by dsp_linear_slope_fit_rows
struct FitArgs {
    const void* wf;
    int64_t n_wf, row_stride;
    int32_t wf_len, n_scan;  // samples per row; samples that have to be visited (the NaN rules of bl_subtract / pole_zero look at all)
    const void* sub;         // per-row value subtracted first (device column) or null: sub_const
    int32_t sub_dtype, sub_mode;  // 0 nothing, 1 bl_subtract (NaN anywhere -> NaN waveform), 2 numpy.subtract (sample by sample)
    double sub_const;
    int32_t has_pz, pz_nan;
    double pz_c;
    int32_t n_fits;
    int32_t stage[DSP_FIT_MAX], first[DSP_FIT_MAX], count[DSP_FIT_MAX];
    void* out;  // [n_fits][4][n_wf] of the compute type: mean, stdev, slope, intercept
};

// arguments of the energy-chain kernels (dsp_energy.hip), filled by the planner when a program has that shape:
//   LOAD [-> BL_SUBTRACT] -> POLE_ZERO -> TRAP_PICKOFF -> STORE_SCALAR
struct EnergyArgs {
    const void* wf;        // waveform rows
    int64_t wf_stride;     // elements between rows
    int32_t wf_offset;     // first sample used
    int32_t len;           // samples per waveform
    const float* bl;       // per-waveform baseline column, or nullptr
    int64_t bl_stride;
    float bl_const;
    int32_t has_bl;        // 0: the chain has no bl_subtract (bl_const is then 0: x - 0 == x exactly)
    const float* tp;       // per-waveform pick-off time column, or nullptr
    int64_t tp_stride;
    float tp_const;
    int32_t mode;          // pick-off mode char
    float* out;
    int64_t out_stride;
    double c;              // exp(-1/tau)
    double rr, ll;         // rise, fall as float64
    int32_t tau_nan;
    int32_t all_nan;       // trap_filter with rise == 0
    int32_t C, pitch;      // samples per lane, C + 1
    float invC;
    int32_t q[3], rho[3];  // lag = q*C + rho
    int32_t lds_elems_per_wave;
    int32_t slot_off;      // element offset of the slot inside the wave's region (2*pitch guard below it)
    const float* tau;      // or null: the pole-zero time constant per event (a column) instead of c / tau_nan -- the TAU builds of the register-resident kernel
    int64_t tau_stride;
    int32_t ablate;        // diagnostic build only (-DDSPEED_HIP_DIAG, libdspeed_hip_diag.so): bit 0/1/2 = skip pass 1/2/3 (results are then
                           // wrong), bit 3 = per-phase cycle stamps.  The product library ignores the field: ABLATE in dsp_energy.hip is a constant 0.
};

// Carry plan of the register-resident energy kernel's pad-free layout (C = len/64 + 2 samples per lane, sample i at LDS element i): for lag
// k and replay sub-chain s the speculative carry needs the float32 prefix sum of the first r samples of the chunk of the lane `shift` below.
// The prefix is pass 2's group-end sum in front of the 8-sample group that holds sample r - 1, plus the first pn samples of that
// group.  Row-invariant, built by the planner (dsp_internal_plan_energy_carries in dsp_plan.cpp, which the CPU can test) in the form the
// kernel uses as it stands.
struct EnergyPlan {       // [lag][replay sub-chain]
    int32_t shift[3][4];  // lane distance
    int32_t cs[3][4];     // sub-chain that holds the capture point, and ...
    int32_t local[3][4];  // ... the samples of it in front of the point (the plan as the planner's checks read it; the kernel uses the form below)
    int32_t grp[3][4];    // element offset, from the start of the lane's chunk, of the group's four pairs (8 * group; group NG: the two-sample tail)
    int32_t side[3][4];   // group whose end sum is the sum of the groups in front (the kernel keeps the group-end sums in registers), -1: none (group 0), 0.0f
    int32_t pn[3][4];     // samples of the group in front of the capture point, 0 .. 8
};

// arguments of the lane-per-waveform chain kernel (dsp_rows.hip), filled by dsp_chain_execute when a program has that shape
struct RowsArgs {
    const void* wf;          // rows
    int64_t wf_stride;       // elements between rows
    int32_t wf_offset, len;  // first sample used, samples per waveform (a multiple of 8)
    int32_t in_kind;         // 0 float32, 1 int16, 2 uint16 rows
    int32_t sub_mode;        // 1: bl_subtract first
    const float* bl;         // per-row baseline column or null: bl_const
    int64_t bl_stride;
    float bl_const;
    int32_t pz_kind;         // 1 pole_zero, 2 double_pole_zero
    int32_t pz_param_nan;    // a NaN time constant: everything downstream is NaN
    double pz_c;             // pole_zero: exp(-1/tau)
    double n1, n2, d1, d2;   // double_pole_zero: numerator / denominator coefficients (pole_zero.py:168-174)
    int32_t trap_kind;       // 0 trap_filter, 1 trap_norm, 2 asym_trap_filter
    int32_t rise_pow2;       // rise is a power of two: x / rise == x * (1 / rise) exactly
    int32_t lag[3];
    int32_t trap_all_nan;    // trap_filter with rise == 0
    double rr, ll, inv_rr, inv_ll;
    void* out_mm[4];         // t_min, t_max, a_min, a_max columns (null: not requested)
    int64_t out_mm_stride[4];
    int32_t tpt_mode;        // 0 none, 1 backward from a known start, 2 backward from the arg-extremum, 3 / 4 the same walking forward
    int32_t tpt_use_min;     // the start is t_min (else t_max)
    const float* thr;        // threshold column or null: thr_const
    int64_t thr_stride;
    const float* ts;         // start column or null: ts_const (modes 1, 3)
    int64_t ts_stride;
    float thr_const, ts_const;
    int32_t walk_nan, walk_frac;  // walk_forward is NaN (output NaN) / not an integer (DSPFatal)
    void* out_tpt;
    int64_t out_tpt_stride;
    int32_t dwt_level, dwt_part;  // Haar level (0: none, else 3..8), 'a' or 'd'
    void* dwt_out;
    int64_t dwt_stride;
    int32_t ring_entries;    // R: history samples kept per lane, a multiple of 8, >= largest lag + 16
    // 1: nothing behind the start of a backward walk matters -- the only output is a walk backward from a known start and the rows are
    // NaN-free or NaN from the first sample on (DSP_OP_LOAD ip[2]): the group stops at the block behind its 64 rows' latest start
    int32_t stop_at_start;
};

// arguments of the lane-per-waveform current-branch kernel (dsp_current.hip), filled by dsp_chain_execute when a program has that shape:
//   LOAD -> WINDOWER -> AVG_CURRENT -> UPSAMPLER -> MOVING_WINDOW_MULTI (3 alternating windows) -> MIN_MAX -> STORE_SCALARs
struct CurrentArgs {
    const void* wf;          // float32 rows
    int64_t wf_stride;
    int32_t wf_offset, n_in; // first sample, samples per row (a multiple of 4)
    const float* t0;         // window start column or null: t0_const
    int64_t t0_stride;
    float t0_const;
    int32_t win_len;         // samples of the window
    int32_t ac_lag;          // avg_current: int(length)
    float ac_length;
    int32_t n_c;             // samples of the current waveform: win_len - ac_lag
    int32_t up_shift, up_half;  // upsampling factor 1 << up_shift, floor(factor / 2)
    int32_t n_up;            // samples of the upsampled waveform (a multiple of 16)
    int32_t ma_len;          // moving-window length (a multiple of 16, at most 112)
    float ma_length;
    int32_t scan_rows;       // 1: the kernel screens the whole rows for NaN; 0: a NaN anywhere means NaN everywhere (DSP_OP_LOAD ip[2])
    void* out[4];            // t_min, t_max, a_min, a_max columns (null: not requested)
    int64_t out_stride[4];
    float* scratch;          // scratch_per_wave floats per resident wavefront: the current waveform and the checkpoints of two passes
    int64_t scratch_per_wave;
};

// arguments of the pole-zero rows kernel (dsp_pz.hip):  LOAD -> [BL_SUBTRACT] -> POLE_ZERO (constant tau) -> STORE
struct PzArgs {
    const void* wf;          // float32 / int16 / uint16 rows, 16-byte aligned
    int64_t wf_stride;
    int32_t wf_offset, len;  // first sample, samples (a multiple of 8)
    int32_t in_kind;         // 0 float32, 1 int16, 2 uint16
    int32_t sub_mode;        // 1: bl_subtract first
    const float* bl;         // per-row baseline column or null: bl_const
    int64_t bl_stride;
    float bl_const;
    int32_t tau_nan;
    double c;                // exp(-1/tau)
    void* out;               // float32 rows
    int64_t out_stride;
    const float* tau;        // or null: the time constant per event (a float32 column) instead of c / tau_nan
    int64_t tau_stride;
    float* row_scale;        // or null: what dsp_fir_f16_rows_kernel would find on the rows written here (FirF16Taps), for a float16 FIR behind
    uint32_t* row_flags;
    void* mm_out[4];         // or null each: min_max (min_max.py:11-82) of the rows as they are READ (t_min, t_max, a_min, a_max; float32 columns)
    int64_t mm_stride[4];
    int32_t mm_on, pad_;
    // or null: what dsp_fir_f16_rows_kernel would find on samples [in_lo, in_hi) of the rows READ here, minus the baseline -- for a float16 FIR
    // that filters that slice of the same rows with the same baseline (the cusp filter of the Ge recipes: waveform[0:6092] - baseline)
    float* in_scale;
    uint32_t* in_flags;
    int32_t in_lo, in_hi;
};

// arguments of the streaming reductions (dsp_reduce.hip), filled by dsp_chain_execute when a program has the shape
//   LOAD -> {MIN_MAX | AMAX | PICKOFF at a constant integral time | TIME_POINT_THRESH from a constant sample or from the extremes}+ -> STORE_SCALARs
#define DSP_REDUCE_PICKS 4
#define DSP_REDUCE_WALKS 6
struct ReduceArgs {
    const void* wf;          // float32 / int16 / uint16 rows
    int64_t wf_stride;
    int32_t wf_offset, len;  // first sample, samples
    void* out[5];            // t_min, t_max, a_min, a_max of MIN_MAX, the maximum of AMAX (null: not requested); float32 columns
    int64_t out_stride[5];
    void* pick_out[DSP_REDUCE_PICKS];
    int64_t pick_stride[DSP_REDUCE_PICKS];
    int32_t pick_at[DSP_REDUCE_PICKS];    // sample index, -1: outside the waveform (NaN)
    int32_t pick_rule[DSP_REDUCE_PICKS];  // 1: fixed_time_pickoff (a NaN anywhere in the row -> NaN), 0: the plain sample
    // time_point_thresh walks that start at a constant sample or at the minimum / maximum found above
    void* walk_out[DSP_REDUCE_WALKS];
    int64_t walk_stride[DSP_REDUCE_WALKS];
    const float* walk_thr[DSP_REDUCE_WALKS];  // threshold column, or null: walk_thr_const
    int64_t walk_thr_stride[DSP_REDUCE_WALKS];
    float walk_thr_const[DSP_REDUCE_WALKS];
    int32_t walk_from[DSP_REDUCE_WALKS];      // 0: walk_start, 1: t_min, 2: t_max, 3: the column walk_ts, 4 + j: where walk j (an earlier one) ended
    int32_t walk_start[DSP_REDUCE_WALKS];
    int32_t walk_forward[DSP_REDUCE_WALKS];
    // round 4: the rise-time walks of a recipe as a launch of their own behind its program (thousands of rows in flight instead of four a CU) --
    // thresholds that are a fraction of a per-event value (the column times walk_thr_factor: one float multiplication, as SCALAR_AFFINE makes it),
    // starts that are a column or where an earlier walk ended (checked like the processor's: DSPFatal for a fractional or outside start)
    float walk_thr_factor[DSP_REDUCE_WALKS];
    int32_t walk_thr_scaled[DSP_REDUCE_WALKS];
    const float* walk_ts[DSP_REDUCE_WALKS];
    int64_t walk_ts_stride[DSP_REDUCE_WALKS];
    int32_t n_walks;
    int32_t need_stream;  // 0: nothing asks for the whole row (walks only, on rows that are NaN from the first sample on or NaN-free: LOAD ip[2])
};

// arguments of the peak finder (dsp_extrema.hip), filled by the planner when a program has the shape
//   LOAD -> MULTI_EXTREMA -> STORE, STORE, STORE_SCALAR, STORE_SCALAR
#define DSP_EXTREMA_UNION_MAX 64 /* search_direction 3 keeps a sweep's tags one per lane: the longest list it takes */
struct ExtremaArgs {
    const void* wf;          // float32 / int16 / uint16 rows (the float32 loop) or float64 / int32 / uint32 rows (the float64 loop)
    int64_t wf_stride;
    int32_t wf_offset, len;  // first sample, samples
    int32_t m;               // length of vt_max_out / vt_min_out
    int32_t direction;       // search_direction: 0 forward, 1 backward, 3 the union of both
    const void* par[4];      // a_delta_max_in, a_delta_min_in, a_abs_max_in, a_abs_min_in: a column of the loop's type, or null: par_const
    int64_t par_stride[4];
    double par_const[4];
    void* vt_out[2];         // vt_max_out, vt_min_out: rows of m values of the loop's type
    int64_t vt_stride[2];
    uint32_t* n_out[2];      // n_max_out, n_min_out
    int64_t n_stride[2];
};

// arguments of the histogram kernel (dsp_hist.hip), filled by the planner when a program has one of the shapes
//   LOAD -> HISTOGRAM -> STORE, STORE
//   LOAD -> HISTOGRAM -> HISTOGRAM_STATS [-> STORE, STORE] -> STORE_SCALAR x 3
//   LOAD, LOAD -> HISTOGRAM_STATS -> STORE_SCALAR x 3          (weights and edges read from memory)
// A wavefront keeps a uint32 counter per bin in its own LDS region, four regions to a workgroup: 2048 bins are 32 KiB a workgroup, five
// workgroups (20 wavefronts, five per SIMD) in a CU's 160 KiB; 100 bins leave the register file as the only bound.
#define DSP_HIST_MAX_BINS 2048
struct HistArgs {
    const void* wf;          // histogram: float32 / int16 / uint16 rows (the float32 loop) or float64 rows (the float64 loop); null: stats alone
    int64_t wf_stride;
    int32_t wf_offset, len;
    int32_t m;               // bins: len(weights); the borders are m + 1
    int32_t stats;           // histogram_stats runs on the counters (fused) or on w_in / e_in (alone)
    int32_t max_blocks;      // histogram: rows are dealt out to at most this many workgroups (0: up to 8192)
    void* w_out;             // weights_out rows, or null: not stored
    void* b_out;             // borders_out rows, or null
    int64_t w_stride, b_stride;
    const void* w_in;        // stats alone: weights_in / edges_in rows of the loop's type
    const void* e_in;
    int64_t w_in_stride, e_in_stride;
    int32_t w_in_offset, e_in_offset;
    const void* max_in;      // a column of the loop's type, or null: max_in_const
    int64_t max_in_stride;
    double max_in_const;
    void* s_out[3];          // mode_out, max_out, fwhm_out
    int64_t s_stride[3];
};

// arguments of the threshold kernel (dsp_thresh.hip), filled by the planner when a program has one of the shapes
//   LOAD -> [LOAD of the thresholds ->] MULTI_TIME_POINT_THRESH -> STORE
//   LOAD -> TIME_OVER_THRESHOLD -> STORE_SCALAR
// A wavefront keeps the row's thresholds one per lane (ranked, then in ascending order) and a result per lane: nothing lives in LDS.
#define DSP_THRESH_MAX 64 /* thresholds of one multi_time_point_thresh */
struct ThreshArgs {
    const void* wf;          // float32 / int16 / uint16 rows (the float32 loop) or float64 rows (the float64 loop)
    int64_t wf_stride;
    int32_t wf_offset, len;  // first sample, samples (multi_time_point_thresh: at least 2)
    int32_t m;               // thresholds of multi_time_point_thresh; 0: time_over_threshold
    int32_t polarity;        // +1 or -1
    int32_t mode;            // interpolation mode, a character of "iafbcrnl"
    const void* thr;         // multi_time_point_thresh: lists of m values of the loop's type, thr_stride apart (0: one list for every row);
    int64_t thr_stride;      //   time_over_threshold: a column of the loop's type, or null: thr_const
    int32_t thr_offset;
    double thr_const;
    const void* ts;          // t_start: a column of the loop's type, or null: ts_const
    int64_t ts_stride;
    double ts_const;
    void* out;               // t_out rows of m values, or the count, one value per row; the loop's type
    int64_t out_stride;
};

// arguments of the spectrum kernel (dsp_spectrum.hip), filled by the planner when a program has one of the shapes
//   LOAD -> PSD -> STORE
//   LOAD -> FFT -> STORE
// One row is one transform of `points` complex points (a power of two) held in LDS: a power-of-two row packed as len / 2 points and unpacked
// behind the transform, any other row Bluestein's convolution of the next power of two >= 2 len - 1.  The tables are the chain's, written
// once when it is created (dsp_spectrum_tables.h); (re, im) pairs of the loop's type.
#define DSP_SPECTRUM_F32_POW2_MAX 16384 /* samples of a power-of-two row, float32 loop (the float64 loop: half): 64 KiB of LDS a row */
#define DSP_SPECTRUM_F32_ANY_MAX 4096   /* samples of any other row, float32 loop (the float64 loop: half) */
struct SpectrumArgs {
    const void* wf;          // float32 / int16 / uint16 rows (the float32 loop) or float64 rows (the float64 loop)
    int64_t wf_stride;
    int32_t wf_offset, len;  // first sample, samples
    int32_t m;               // bins: len / 2 + 1
    int32_t complex_out;     // 1: fft (2 m values a row), 0: psd
    int32_t points, log2_points;  // the transform in LDS
    int32_t bluestein;       // 0: len is a power of two
    int32_t wide;            // 1: a workgroup of 256 per row, 0: a wavefront per row, four rows to a workgroup
    const void* twiddle;     // exp(-2 pi i k / points), k < points / 2
    const void* aux;         // power of two: exp(-2 pi i k / len), k <= len / 2 (the unpacking step); Bluestein: the chirp exp(-i pi j^2 / len), j < len
    const void* filter;      // Bluestein: the spectrum of the conjugate chirp over `points`, in bit-reversed order
    void* out;
    int64_t out_stride;
};

// arguments of the sorting kernel (dsp_sort.hip), filled by the planner when a program has the shape
//   LOAD -> SORT -> STORE
// One row is `padded` order-preserving unsigned keys in LDS (dsp_kernels.h, dsp_sort), the keys past `len` +inf's.
#define DSP_SORT_F32_MAX 16384 /* samples of a row, float32 loop (the float64 loop: half): 64 KiB of LDS a row */
struct SortArgs {
    const void* wf;          // float32 / int16 / uint16 rows (the float32 loop) or float64 rows (the float64 loop)
    int64_t wf_stride;
    int32_t wf_offset, len;  // first sample, samples
    int32_t padded;          // dsp_sort::padded(len): the power of two the network runs over
    int32_t wide;            // 1: a workgroup of 256 per row, 0: a wavefront per row, four rows to a workgroup
    void* out;               // rows of len samples of the loop's type
    int64_t out_stride;
};

// arguments of the resampling kernel (dsp_interp.hip), filled by the planner when a program has the shape
//   LOAD -> INTERP_UPSAMPLE -> STORE
// The row lives in LDS in the loop's type; mode 's' keeps its second derivatives as float64 behind it (dsp_kernels.h, dsp_interp).
#define DSP_INTERP_F32_MAX 16384       /* samples of a row, float32 loop (the float64 loop: half): 64 KiB of LDS a row */
#define DSP_INTERP_SPLINE_F32_MAX 5456 /* mode 's', float32 loop: 12 bytes a sample */
#define DSP_INTERP_SPLINE_F64_MAX 4096 /* mode 's', float64 loop: 16 bytes a sample */
struct InterpArgs {
    const void* wf;          // float32 / int16 / uint16 rows (the float32 loop) or float64 rows (the float64 loop)
    int64_t wf_stride;
    int32_t wf_offset, len;  // first sample, samples (n)
    int32_t out_len;         // m: the resampling ratio is m / n, a float64
    int32_t mode;            // 'i' 'n' 'f' 'c' 'l' 'h' 's'
    int32_t wide;            // 1: a workgroup of 256 per row, 0: a wavefront per row, four rows to a workgroup
    int32_t out_vec;         // 1: 16-byte stores (the output rows' start and stride are whole vectors: set per call)
    void* out;               // rows of out_len samples of the loop's type
    int64_t out_stride;
};

// arguments of the dense-layer kernel (dsp_dense.hip), filled by the planner when a program has one of the shapes
//   LOAD -> [NORMALISE ->] DENSE -> STORE | STORE_SCALAR        LOAD -> NORMALISE -> STORE
// Rows and weights pass through LDS in chunks along n (dsp_kernels.h, dsp_dense); the accumulators stay in registers.
#define DSP_DENSE_N_MAX 16384 /* inputs of a layer */
#define DSP_DENSE_M_MAX 256   /* outputs of a layer: 16 column blocks of accumulators a wavefront */
#define DSP_DENSE_LIMITS_TEXT "layers of up to %d inputs and %d outputs"
struct DenseArgs {
    const void* wf;          // float32 / int16 / uint16 rows (the float32 loop) or float64 rows (the float64 loop)
    int64_t wf_stride;
    int32_t wf_offset, len;  // first sample, samples (n)
    int32_t m;               // outputs (1: the classification form too); 0: no DENSE, the normalised row itself is stored
    int32_t activation;      // the character; none of "srlmt": NaN outputs
    int32_t normalise;       // 1: (x - means) / sqrt(variances) while a row is staged
    int32_t pad_;
    const void* weights;     // (n, m) row-major, the loop's type
    const void* bias;        // m values or null
    const void* means;       // n values each (normalise)
    const void* variances;
    void* out;               // rows of m values (of n: m == 0) of the loop's type
    int64_t out_stride;
};

// arguments of the support-vector classifier's kernel (dsp_svm.hip), filled by the planner when a program has the shape
//   LOAD -> SVM_PREDICT -> STORE_SCALAR
// Rows and support vectors pass through LDS in chunks along n (dsp_kernels.h, dsp_svm); both products and the decisions stay in registers.
// The model is float64 in both loops: the reference casts the row up and libsvm works in float64.
#define DSP_SVM_CLASSES_MAX 23 /* classes of a model: 253 pairs, 16 blocks of decision accumulators a wavefront */
#define DSP_SVM_LIMITS_TEXT "rows of up to %d samples and models of up to %d classes"
#define DSP_SVM_MODEL_MAX (1 << 28) /* support-vector samples (n_sv * n) and coefficients (n_sv * P): the longest binding a chain takes */
#define DSP_SVM_MODEL_TEXT "at least one support vector, and at most %d support-vector samples and coefficients (%d support vectors of %d samples, %d pairs of classes given)"
struct SvmArgs {
    const void* wf;          // float32 rows (either loop) or float64 rows (the float64 loop)
    int64_t wf_stride;
    int32_t wf_offset, len;  // first sample, samples (n)
    int32_t n_sv;            // support vectors, grouped by class in class order
    int32_t n_classes;       // k
    int32_t n_pairs;         // P = k (k - 1) / 2
    int32_t linear;          // 0: K = exp(-gamma |x - sv|^2), 1: K = x . sv
    int32_t f64;             // 1: the float64 loop (the label is a float64)
    int32_t pad_;
    double gamma;
    const double* sv;        // (n_sv, n) row-major
    const double* sv_norm;   // n_sv squared norms, made on the host
    const double* coef;      // D, (n_sv, P) row-major: the coefficient of support vector s in pair p, 0 where its class is not in the pair
    const double* intercept; // P
    const double* classes;   // k class values
    void* label;             // one value of the loop's type per row
    int64_t label_stride;
    double* dec;             // rows of P decisions, or null
    int64_t dec_stride;
};

// arguments of the mirrored-edge FIR kernel (dsp_reflect.hip), filled by the planner when a program has one of the shapes
//   LOAD -> REFLECTED_CONVOLVE -> STORE        LOAD -> REFLECTED_CONVOLVE -> AVG_CURRENT -> STORE [of the filtered row too]
// The row lives in LDS in the loop's type with its mirrored margins beside it (dsp_kernels.h, dsp_reflect).
#define DSP_REFLECT_F32_MAX 16384 /* len + n_taps - 1, float32 loop: 64 KiB of LDS a staged row */
#define DSP_REFLECT_F64_MAX 8192  /* float64 loop */
#define DSP_REFLECT_LIMITS_TEXT "len(w_in) + len(kernel) - 1 of up to %d in the float32 loop and %d in the float64 loop"
struct ReflectArgs {
    const void* wf;          // float32 / int16 / uint16 rows (the float32 loop) or float64 rows (the float64 loop)
    int64_t wf_stride;
    int32_t wf_offset, len;  // first sample, samples (n)
    int32_t n_taps;          // m <= n
    int32_t taps_nan;        // 1: the caller found a NaN among the taps: every row comes out as NaNs
    int32_t wide;            // 1: a workgroup of 256 per row, 0: a wavefront per row, four rows to a workgroup
    int32_t out_vec;         // 1: 16-byte stores of the filtered row (the output rows' start and stride are whole vectors: set per call)
    int32_t lag;             // the fused avg_current: int(length), 0: none
    int32_t pad_;
    double length;           // ... and its divisor, rounded to the loop's type
    const void* taps;        // n_taps values of the loop's type
    void* out;               // rows of len samples of the loop's type, or null: the filtered row is not stored (the fused form)
    int64_t out_stride;
    void* cur;               // rows of len - lag samples (the fused form) or null
    int64_t cur_stride;
};

// arguments of the pile-up kernel (dsp_pileup.hip), filled by the planner when a program has one of the shapes
//   LOAD -> RC_CR2 -> STORE
//   LOAD -> BI_LEVEL_ZERO_CROSSING -> STORE, STORE, STORE_SCALAR
//   LOAD -> RC_CR2 -> BI_LEVEL_ZERO_CROSSING [-> STORE of the filtered row] -> STORE, STORE, STORE_SCALAR
// each with or without a BL_SUBTRACT of the rows, in place, behind the LOAD.  One waveform per lane; the rows pass through an LDS tile of 64 rows x 64 samples (dsp_kernels.h, dsp_pileup).
struct PileupArgs {
    const void* wf;          // float32 / int16 / uint16 rows (the float32 loop) or float64 rows (the float64 loop)
    int64_t wf_stride;
    int32_t wf_offset, len;  // first sample, samples (the filter: more than 3; the walk: at least 1)
    int32_t filter;          // 1: rc_cr2 runs on the row
    int32_t walk;            // 1: bi_level_zero_crossing_time_points runs on the row, or on the filtered row as stored
    int32_t m;               // entries of each list
    int32_t out_vec;         // 1: 16-byte stores of the filtered row (the output rows' start and stride are whole vectors: set per call)
    int32_t tau_nan;         // 1: t_tau is a NaN: every filtered row NaN, no error
    int32_t sub_mode;        // 1: the baseline is subtracted from every sample as it is read (bl_subtract)
    const void* sub;         // the baseline: a column of the loop's type, or null: sub_const
    int64_t sub_stride;
    double sub_const;
    double c1, c2, c3;       // 3a, 3(a a), a(a a) with a = exp(-1 / t_tau): float64, formed on the host
    const void* par[4];      // a_pos_threshold_in, a_neg_threshold_in, gate_time_in, t_start_in: columns of the loop's type, or null: par_const
    int64_t par_stride[4];
    double par_const[4];
    void* out;               // filtered rows of len samples of the loop's type, or null: not stored
    int64_t out_stride;
    void* list[2];           // polarity_out, t_trig_times_out: rows of m values of the loop's type
    int64_t list_stride[2];
    uint32_t* n_out;         // n_crossings_out
    int64_t n_stride;
};

// arguments of the pulse picker (dsp_pulses.hip), filled by the planner when a program has one of the shapes
//   LOAD -> LOAD of the candidates -> PEAK_SNR_THRESHOLD -> STORE of idx_out, STORE_SCALAR of the count
//   LOAD -> LOAD of the positions -> MULTI_A_FILTER -> STORE of va_max_out
//   LOAD -> LOAD of the candidates -> PEAK_SNR_THRESHOLD -> MULTI_A_FILTER [-> STORE of idx_out] -> STORE of va_max_out, STORE_SCALAR
// A wavefront keeps the row's list one entry per lane: nothing lives in LDS.
#define DSP_PEAKS_MAX 64 /* entries of a list of peak_snr_threshold / multi_a_filter (as DSP_THRESH_MAX, and the peak finder's direction 3) */
struct PulsesArgs {
    const void* wf;          // float32 / int16 / uint16 rows (the float32 loop) or float64 rows (the float64 loop)
    int64_t wf_stride;
    int32_t wf_offset, len;  // first sample, samples
    int32_t m;               // entries of the list, 1 .. DSP_PEAKS_MAX
    int32_t pick;            // 1: peak_snr_threshold runs on the list
    int32_t amp;             // 1: multi_a_filter runs on the list, or on the packed list of the picker (registers)
    int32_t width;           // int(width_in), at most len (a wider window is clamped to the row all the same)
    const void* list;        // idx_in / vt_maxs_in: rows of m values of the loop's type
    int64_t list_stride;
    int32_t list_offset;
    const void* ratio;       // ratio_in: a column of the loop's type, or null: ratio_const
    int64_t ratio_stride;
    double ratio_const;
    void* idx_out;           // rows of m values of the loop's type, or null: not stored
    int64_t idx_stride;
    uint32_t* n_out;         // n_idx_out
    int64_t n_stride;
    void* amp_out;           // va_max_out: rows of m values of the loop's type
    int64_t amp_stride;
};

// arguments of the decay-tail fitter (dsp_tailfit.hip), filled by the planner when a program has one of the shapes
//   LOAD -> LOG_CHECK -> STORE
//   LOAD -> POLY_FIT -> STORE of the coefficients
//   LOAD -> LOAD of the coefficients -> POLY_DIFF | POLY_EXP_RMS -> STORE_SCALAR, STORE_SCALAR
//   LOAD -> LOG_CHECK -> POLY_FIT [-> STORE of the logged row] -> STORE of the coefficients
//   LOAD -> LOG_CHECK -> POLY_FIT -> POLY_DIFF | POLY_EXP_RMS [-> STORE of the logged row] [-> STORE of the coefficients] -> STORE_SCALAR, STORE_SCALAR
// each with or without a BL_SUBTRACT of the rows, in place, behind their LOAD.  One waveform per lane; the rows pass through an LDS tile of
// 64 rows x 64 samples (dsp_kernels.h, dsp_tailfit), twice where the residuals follow the fit.
#define DSP_POLY_MAX 8 /* coefficients of poly_fit / poly_diff / poly_exp_rms: a lane keeps as many float64 accumulators */
#define DSP_POLY_MAX_TEXT "at most %d coefficients (%d given): a lane keeps one float64 accumulator each"
#define DSP_POLY_POWER_TEXT \
    "(n - 1)**(m - 1) must stay below 2**63 (n = %d samples, m = %d coefficients): beyond it the reference's int64 power i**j wraps silently"
// does i**j stay an int64 for every sample i < n and every power j < m?
static inline bool dsp_poly_powers_fit(int64_t n, int m) {
    const uint64_t b = n > 1 ? (uint64_t)(n - 1) : 0, top = ((uint64_t)1 << 63) - 1;
    uint64_t p = 1;
    for (int j = 1; j < m; ++j) {
        if (b != 0 && p > top / b) return false;
        p *= b;
    }
    return true;
}
struct TailfitArgs {
    const void* wf;          // float32 / int16 / uint16 rows (the float32 loop) or float64 rows (the float64 loop)
    int64_t wf_stride;
    int32_t wf_offset, len;  // first sample, samples
    int32_t log;             // 1: log_check runs on the row
    int32_t fit;             // 1: poly_fit runs on the row, or on the logged row
    int32_t resid;           // 0: none; 1: poly_diff; 2: poly_exp_rms -- with the coefficients of `pars`, or the fitted ones as stored
    int32_t resid_log;       // 1: the residuals are those of the logged row (else of the row as loaded)
    int32_t m;               // coefficients, 1 .. DSP_POLY_MAX (with fit or resid)
    int32_t out_vec;         // 1: 16-byte stores of the logged row (the output rows' start and stride are whole vectors: set per call)
    int32_t sub_mode;        // 1: the baseline is subtracted from every sample as it is read (bl_subtract)
    const void* sub;         // the baseline: a column of the loop's type, or null: sub_const
    int64_t sub_stride;
    double sub_const;
    const double* inv;       // poly_fit: m * m float64 values, row-major, whatever the loop
    const void* pars;        // poly_diff / poly_exp_rms alone: rows of m coefficients of the loop's type
    int64_t pars_stride;
    int32_t pars_offset;
    void* out;               // logged rows of len samples of the loop's type, or null: not stored
    int64_t out_stride;
    void* pars_out;          // rows of m fitted coefficients of the loop's type, or null: not stored
    int64_t pars_out_stride;
    void* mean_out;          // the two results of the residuals: a value of the loop's type per row
    int64_t mean_stride;
    void* rms_out;
    int64_t rms_stride;
};

// arguments of the waveform aligner (dsp_align.hip), filled by the planner when a program has one of the shapes
//   LOAD -> INL_CORRECTION -> STORE
//   LOAD -> WF_CENTROID -> STORE_SCALAR
//   LOAD -> WF_ALIGNMENT -> STORE
//   LOAD -> WF_CORRECTION -> STORE
//   LOAD -> WF_ALIGNMENT -> WF_CORRECTION [-> STORE of the aligned row] -> STORE of the corrected row
// A wavefront per row, four to a workgroup, nothing in LDS (dsp_pulses.hip's geometry).
enum { DSP_ALIGN_INL = 1, DSP_ALIGN_CENTROID = 2, DSP_ALIGN_WINDOW = 3, DSP_ALIGN_CORRECT = 4 };
struct AlignArgs {
    const void* wf;           // the rows: see DSP_OP_WF_ALIGNMENT (dspeed_hip.h) for the types each op takes
    int64_t wf_stride;
    int32_t wf_offset, len;   // first sample, samples
    int32_t mode;             // DSP_ALIGN_*: the first op of the launch
    int32_t f64;              // 1: the float64 loop (the rows' type alone does not tell: int32 rows feed both)
    int32_t out_vec;          // 1: 16-byte stores of the streamed outputs (their start and stride are whole vectors: set per call)
    int32_t correct;          // with DSP_ALIGN_WINDOW: 1, the template is subtracted from the window before it is stored
    const void* table;        // inl (DSP_ALIGN_INL) or w_corr: table_len values of the loop's type
    int32_t table_len;
    int32_t start, stop;      // wf_correction: the template is subtracted on [start, stop) of the row it reads
    const int* table_nan;     // device word: nonzero, the table holds a NaN (written by the scan that runs ahead of the launch); set per call
    const void* centroid;     // wf_alignment: a column of the loop's type, or null: centroid_const
    int64_t centroid_stride;
    double centroid_const;
    double shift;             // get_wf_centroid, wf_alignment: as the loop receives it
    int32_t size;             // wf_alignment: samples of the window
    void* out;                // rows of the loop's type: inl_correction's, wf_correction's, or the aligned row's (null: not stored)
    int64_t out_stride;
    void* out2;               // the corrected row behind an alignment in the same launch
    int64_t out2_stride;
    void* scalar_out;         // get_wf_centroid: a value of the loop's type per row
    int64_t scalar_stride;
};

// ---- wf_alignment.py:80-87, the rule of a row: shared by the kernel, the planner's constant case and the tests' host program.
// c, sh, s: centroid, shift, size as the loop receives them; all arithmetic in float64, int() truncating (the centroid is no NaN).
//   kind 1  w_out = w_in[first : first + s]
//   kind 2  w_out[:fill] = w_in[0], w_out[fill:] = w_in[:count]   (fill + count == s, count may be 0; count == 1 may also stand for
//           NumPy's broadcast of one sample over s - fill places: count_bcast)
//   kind 3  w_out = w_in[:s]
//   kind 0  the two sides of line 85 differ in length and do not broadcast: the reference raises in NumPy; a NaN row here
struct AlignWindow {
    int kind, first, fill, count;
};
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline AlignWindow dsp_align_window(double c, double sh, int s, int n) {
    const double half = (double)s / 2;
    AlignWindow w = {3, 0, 0, 0};
    if (c >= half && c < (double)n - half) {
        w.kind = 1;
        w.first = (int)(c - half);
    } else if (c > half - sh && c < half) {
        // (c > s/2 - sh >= s/2 - n: both casts stay far inside an int)
        const long long ss = (long long)(((double)s + 1) / 2 - c), k = (long long)(c + half);
        const long long lhs = ss >= s ? 0 : s - ss;                              // len(w_out[ss:]), ss >= 0 since c < s/2
        const long long rhs = k >= 0 ? (k < n ? k : n) : (n + k > 0 ? n + k : 0);  // len(w_in[:k])
        w.kind = (lhs == rhs || rhs == 1) ? 2 : 0;
        w.fill = (int)(s - lhs);
        w.count = (int)rhs;
    }
    return w;
}

// arguments of the matrix-core FIR kernel (dsp_fir_mfma.hip): convolve_wf 'v' + numpy.amax of up to DSP_FIR_MAXK kernels on one waveform
#define DSP_FIR_MAXK 4
struct FirArgs {
    const void* wf;
    int64_t wf_stride;       // elements between rows
    int32_t wf_offset, n;    // first sample, samples of the slice the kernels run over
    int32_t in_kind;         // 0 float32, 1 int16, 2 uint16 rows
    int32_t sub_mode;        // 1: bl_subtract first
    const float* bl;
    int64_t bl_stride;
    float bl_const;
    int32_t n_kernels;
    const float* taps[DSP_FIR_MAXK];  // the kernels as the recipe holds them (np.convolve flips them)
    int32_t m[DSP_FIR_MAXK], p[DSP_FIR_MAXK];  // taps, valid outputs n - m + 1
    void* out[DSP_FIR_MAXK];
    int64_t out_stride[DSP_FIR_MAXK];
    int32_t kend;            // samples the product runs over: a multiple of 32, <= the row's length
    int32_t scan_before, scan_after;  // samples before / after the slice that are screened for NaN (DSP_OP_LOAD ip[0..1])
    int32_t store;           // 1: ONE kernel whose p[0] outputs are written to out[0] as a waveform (dsp_fir_store_kernel), any mode
    int32_t dshift;          // store: output c is the sum over samples c - dshift .. c - dshift + m - 1 ('v' 0, 's' m / 2, 'f' m - 1)
    const uint32_t* row_flags;  // dsp_fir_fixup_kernel: the rows' flags when something has looked at the rows already (dsp_fir_f16.hip), else null
};

// the float16 tap images of dsp_fir_f16.hip (one per kernel: 16 shifted / split copies of tz halfs, then the inverse scale), chain-owned
struct FirF16Taps {
    const void* taps16[DSP_FIR_MAXK];
    int32_t tz;
    const void* row_scale;  // float per row: the power of two that brings the row's largest magnitude into [2^14, 2^15)
    const void* row_flags;  // uint32 per row: bit 0 an infinity, bit 1 a NaN
    int32_t rows_done;      // the kernel that wrote the rows left both already (dsp_pz.hip): no pass over the rows for them
    int32_t pad_;
};


// the run-length FIR of dsp_fir_runs.hip: a kernel that is piecewise constant (the t0 filter of the Ge recipes: a ramp of 8 taps and a
// plateau of 125) written as  sum_b weight[b] * P[c + start + 1 - t[b]]  over its breakpoints t[0] = 0 < t[1] < .. < t[n_break - 1] = m,
// P the float64 prefix sums of the row.  Written by dsp_fir_runs_prep_kernel from the taps binding ahead of every launch.
#define DSP_FIR_RUNS_MAX 24      /* runs a kernel may have (breakpoints: one more) */
#define DSP_FIR_RUNS_MAX_TAPS 512
#define DSP_FIR_RUNS_GROUP 8     /* breakpoints at consecutive taps are taken together, up to this many */
struct FirRunsTable {
    int32_t n_break;   // 0: the taps are not of this form after all (more runs, a NaN or an infinity among them): every row tap by tap
    int32_t taps_nan;  // a NaN among the taps: every output NaN (convolutions.py:45-46)
    int32_t t[DSP_FIR_RUNS_MAX + 2];
    double weight[DSP_FIR_RUNS_MAX + 2];
    // breakpoints at consecutive taps (a ramp: every tap differs from the one before) as groups: first[k] .. first[k] + count[k] - 1
    int32_t n_groups, pad_;
    int32_t first[DSP_FIR_RUNS_MAX + 2], count[DSP_FIR_RUNS_MAX + 2];
};

// arguments of dsp_fir_runs_kernel:  LOAD -> CONVOLVE (any mode, ip[2] = 1) -> [STORE] -> the reductions of ReduceArgs on the filtered waveform
struct FirRunsArgs {
    const float* wf;         // float32 rows, 16-byte aligned
    int64_t wf_stride;
    int32_t wf_offset, n;    // first sample, samples (a multiple of 8)
    const float* taps;       // the kernel as the recipe holds it
    int32_t m, p;            // taps, outputs
    int32_t start;           // output c is np.convolve's full output c + start ('f' 0, 's' (m - 1) / 2, 'v' m - 1)
    int32_t keep;            // 1: the filtered waveform is an output (out), 0: it lives in the wavefront's scratch row until the reductions are done
    float* out;              // float32 rows (keep) or the scratch area: p_pitch floats per resident wavefront
    int64_t out_stride;      // keep: elements between rows; else p_pitch
    const FirRunsTable* table;
    int32_t has_red, pad_;
    ReduceArgs red;          // (wf / wf_stride / wf_offset unused: the reductions read the filtered row)
};
