// dsp_plan.h -- the planner's half of a chain: what dsp_chain_create decides about a dsp_op program WITHOUT touching the device.
//
// dsp_plan_build validates the program (every constant-only DSPFatal condition of the reference included), evaluates the constants the
// reference evaluates once per call, packs the waveform slots into LDS by lifetime, matches the program against the specialised kernels'
// shapes and picks the launch geometry.  It makes no HIP call and includes no HIP header: the same translation unit is compiled for the
// CPU with -fsanitize=address,undefined and fuzzed there (tests/test_planner_fuzz.py, tests/planner_fuzz.cpp).  dsp_host.cpp puts the
// device resources on top (struct dsp_chain : ChainPlan).  The argument blocks it fills are dsp_program.h's, the kernels' LDS geometry and
// the routes dsp_kernels.h's: nothing of the kernels' side is declared here.  Internal header; the public contract is include/dspeed_hip.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "dsp_kernels.h"
#include "dsp_program.h"

constexpr int LDS_BYTES_PER_CU = 160 * 1024;

// Where a kernel that streams rows from memory (dsp_row_stream.h) finds them: the binding of the rows, their type, and whether strides, offsets
// and length are whole 16-byte vectors (the launch adds the alignment of the pointer it is handed)
struct RowSource {
    int io = -1;
    int dtype = DSP_F32;
    bool vec = false;
};

// (dsp_plan.cpp; exported for the CPU tests)
extern "C" void dsp_internal_plan_energy_carries(int Ci, int S, const int32_t* lags, EnergyPlan* plan);

// thread-local text behind dsp_last_error(); dsp_fail formats it and hands `code` back
int dsp_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
void dsp_set_last_error(const char* text);
const char* dsp_plan_last_error();
int dsp_elem_size(int dtype);

// Everything the planner decides.  Plain data apart from the note; the pointers inside the kernels' argument blocks stay null here (the
// I/O pointers of a launch are filled in by dsp_chain_execute, the device images of the float16 FIR taps by dsp_chain_create).
struct ChainPlan {
    DevProgram host{};
    int lds_bytes_per_wave = 0;
    int waves_per_block = 0;   // generic VM launch
    int classic_wpb = 0;       // classic energy kernel launch (built for 2 wavefronts per SIMD)
    bool has_fir = false;      // the program holds a CONVOLVE: the VM build with the FIR op (2 wavefronts per SIMD instead of 4)
    bool f64 = false;  // the float64 gufunc loop (LDS elements are 8 bytes)
    bool i64 = false;  // an integer program of per-event values (compute_dtype DSP_I64): the row-per-lane kernel with 64-bit integer registers
    // specialised energy-chain kernel (dsp_energy.hip), selected when the program has exactly that shape
    bool fused_ok = false, fused_on = true;
    EnergyArgs fused{};
    int fused_trap = 0, fused_npf = 0, wf_dtype = DSP_F32;
    // register-resident kernel (pad-free LDS image): the default for 1024/2048/4096-sample energy chains
    bool rr_ok = false;
    // 6: register-resident kernel (default where it applies), 8: the same with two replay sub-chains per lane (A/B only),
    // 1: classic kernel (VM layout, bit-identical to the VM)
    int variant = 1;
    EnergyArgs rr{};
    EnergyPlan plan[2]{};  // [S - 1]
    int rr_lds_bytes = 0;
    int io_wf = -1, io_bl = -1, io_tp = -1, io_out = -1, io_tau = -1;
    // lane-per-waveform kernel (dsp_rows.hip): [bl_subtract ->] pole_zero | double_pole_zero -> short trapezoid -> min_max /
    // time_point_thresh, + Haar DWT of the pole-zero corrected waveform
    bool rows_ok = false;
    RowsArgs rows{};
    int rows_lds_bytes = 0;
    int rio_wf = -1, rio_bl = -1, rio_thr = -1, rio_ts = -1, rio_mm[4] = {-1, -1, -1, -1}, rio_tpt = -1, rio_dwt = -1;
    // matrix-core FIR kernel (dsp_fir_mfma.hip): LOAD [-> BL_SUBTRACT] -> CONVOLVE_AMAX ('v') x 1..4 -> STORE_SCALARs
    bool fir_ok = false;
    FirArgs fir{};
    int fir_lds_bytes = 0;
    int fio_wf = -1, fio_bl = -1, fio_taps[DSP_FIR_MAXK] = {-1, -1, -1, -1}, fio_out[DSP_FIR_MAXK] = {-1, -1, -1, -1};
    // the amax form on the float16 matrix instructions (dsp_fir_f16.hip): the default where the rows keep 16-byte alignment
    bool fir_f16 = false;
    FirF16Taps f16{};  // device images of the kernels' taps (rewritten by every launch: the taps are a binding), the rows' scales and flags
    // why a program that all but has the shape of a specialised kernel runs on the interpreter instead (dsp_chain_kernel_note)
    std::string note;
    // a program of scalar ops only (dsp_scalar.hip: a row per lane)
    bool scalar_ok = false;
    // lane-per-waveform current-branch kernel (dsp_current.hip)
    bool cur_ok = false;
    CurrentArgs cur{};
    int cur_lds_bytes = 0, cio_wf = -1, cio_t0 = -1, cio_out[4] = {-1, -1, -1, -1};
    // pole-zero rows written back as rows (dsp_pz.hip)
    bool pz_ok = false;
    PzArgs pz{};
    int pio_wf = -1, pio_bl = -1, pio_out = -1, pio_tau = -1, pio_mm[4] = {-1, -1, -1, -1};
    // streaming reductions of rows (dsp_reduce.hip)
    bool red_ok = false;
    ReduceArgs red{};
    RowSource red_src{};
    int dio_out[5] = {-1, -1, -1, -1, -1}, dio_pick[DSP_REDUCE_PICKS] = {-1, -1, -1, -1};
    int dio_walk[DSP_REDUCE_WALKS] = {-1, -1, -1, -1, -1, -1}, dio_walk_thr[DSP_REDUCE_WALKS] = {-1, -1, -1, -1, -1, -1},
        dio_walk_ts[DSP_REDUCE_WALKS] = {-1, -1, -1, -1, -1, -1};
    // The ops no interpreter case stands behind: a program that holds one runs on that op's kernel or is refused (the table of these routes
    // is dsp_plan.cpp's).  DSP_ROUTE_EXTREMA, DSP_ROUTE_HIST, DSP_ROUTE_THRESH, DSP_ROUTE_SPECTRUM, DSP_ROUTE_SORT, DSP_ROUTE_INTERP, DSP_ROUTE_DENSE, DSP_ROUTE_REFLECT, DSP_ROUTE_PILEUP, DSP_ROUTE_PULSES, DSP_ROUTE_TAILFIT, DSP_ROUTE_ALIGN or DSP_ROUTE_SVM; DSP_ROUTE_VM: the program holds none.
    dsp_route kernel_only = DSP_ROUTE_VM;
    // the peak finder (dsp_extrema.hip): the one kernel a program with MULTI_EXTREMA runs on
    ExtremaArgs ext{};
    RowSource ext_src{};
    int xio_par[4] = {-1, -1, -1, -1}, xio_vt[2] = {-1, -1}, xio_n[2] = {-1, -1};
    // histogram and histogram_stats (dsp_hist.hip): the one kernel a program with HISTOGRAM or HISTOGRAM_STATS runs on
    HistArgs hist{};
    RowSource hist_src{};  // (io < 0: histogram_stats alone, on weights and edges read from rows; dtype: the loop's)
    int hio_w = -1, hio_b = -1, hio_w_in = -1, hio_e_in = -1, hio_max_in = -1, hio_s[3] = {-1, -1, -1};
    // multi_time_point_thresh and time_over_threshold (dsp_thresh.hip): the one kernel a program with either op runs on
    ThreshArgs thresh{};
    RowSource thresh_src{};
    int tio_thr = -1, tio_ts = -1, tio_out = -1;
    // psd and fft (dsp_spectrum.hip): the one kernel a program with either op runs on
    SpectrumArgs spec{};
    RowSource spec_src{};
    int sio_out = -1;
    // sort (dsp_sort.hip): the one kernel a program with the op runs on
    SortArgs sort{};
    RowSource sort_src{};
    int oio_out = -1;
    // interpolating_upsampler (dsp_interp.hip): the one kernel a program with the op runs on
    InterpArgs interp{};
    RowSource interp_src{};
    int iuo_out = -1;
    // the neural-network layers (dsp_dense.hip): the one kernel a program with NORMALISE or DENSE runs on; weights, bias, means, variances, output
    DenseArgs dense{};
    RowSource dense_src{};
    int eio_w = -1, eio_b = -1, eio_mean = -1, eio_var = -1, eio_out = -1;
    // reflected_convolve_wf, with an avg_current of its output or without (dsp_reflect.hip): the one kernel a program with the op runs on
    ReflectArgs reflect{};
    RowSource reflect_src{};
    int rio_taps = -1, rio_out = -1, rio_cur = -1;
    // rc_cr2 and bi_level_zero_crossing_time_points, apart or in one launch (dsp_pileup.hip): the one kernel a program with either op runs on
    PileupArgs pileup{};
    RowSource pileup_src{};
    int lio_par[4] = {-1, -1, -1, -1}, lio_out = -1, lio_list[2] = {-1, -1}, lio_n = -1, lio_sub = -1;
    // peak_snr_threshold and multi_a_filter, apart or in one launch (dsp_pulses.hip): the one kernel a program with either op runs on
    PulsesArgs pulses{};
    RowSource pulses_src{};
    int uio_list = -1, uio_ratio = -1, uio_idx = -1, uio_n = -1, uio_amp = -1;
    // log_check, poly_fit, poly_diff and poly_exp_rms, apart or in one launch (dsp_tailfit.hip): the one kernel a program with any of them runs on
    TailfitArgs tailfit{};
    RowSource tailfit_src{};
    int aio_sub = -1, aio_inv = -1, aio_pars = -1, aio_out = -1, aio_pars_out = -1, aio_mean = -1, aio_rms = -1;
    // inl_correction, get_wf_centroid, wf_alignment and wf_correction, the last two apart or in one launch (dsp_align.hip): the one kernel a program with any of them runs on
    AlignArgs align{};
    RowSource align_src{};
    int gio_table = -1, gio_centroid = -1, gio_out = -1, gio_out2 = -1, gio_scalar = -1;
    // svm_predict (dsp_svm.hip): the one kernel a program with SVM_PREDICT runs on; support vectors, their norms, D, intercepts, classes, label, decisions
    SvmArgs svm{};
    RowSource svm_src{};
    int vio_sv = -1, vio_norm = -1, vio_coef = -1, vio_icpt = -1, vio_cls = -1, vio_label = -1, vio_dec = -1;
    // run-length FIR with the reductions of its output (dsp_fir_runs.hip); the reductions' bindings are dio_* above
    bool runs_ok = false;
    FirRunsArgs runs{};
    int uio_wf = -1, uio_taps = -1, uio_out = -1;
    // LDS packing as decided (for dsp_chain_plan and the fuzzer's invariants): region of slot s = [slot_base[s], slot_base[s] + slot_foot[s])
    // elements of the compute type, alive from op slot_first_op[s] to slot_last_op[s] of the caller's program
    int32_t slot_base[DSP_MAX_SLOTS] = {0}, slot_foot[DSP_MAX_SLOTS] = {0}, slot_first_op[DSP_MAX_SLOTS] = {0}, slot_last_op[DSP_MAX_SLOTS] = {0};
    uint8_t slot_shares[DSP_MAX_SLOTS] = {0};
};

// 0 or the DSP_ERR_* / DSP_E_* code (text in dsp_plan_last_error()); `ch` must be a freshly constructed plan
int dsp_plan_build(ChainPlan* ch, const dsp_op* ops, int n_ops, const dsp_io_desc* io, int n_io, const int32_t* slot_len, int n_slots,
                   int n_sregs, int compute_dtype);
// the route a planned chain takes on rows that keep 16-byte alignment (fused_on and variant included; null: the interpreter)
dsp_route dsp_plan_route(const ChainPlan* ch);
// its kernel: dsp_route_kernel_names (dsp_kernels.h)
const char* dsp_plan_route_kernel_name(dsp_route route);
const char* dsp_plan_kernel_name(const ChainPlan* ch);
// does a specialised kernel's shape stand behind the chain (its note is then not shown)?  The route, but for one case: the classic energy
// kernel asked for (variant 1) on a program only the register-resident one takes runs on the interpreter and still counts
bool dsp_plan_specialised(const ChainPlan* ch);
// a digest of every environment switch dsp_plan_build reads (DSPEED_HIP_FIR_F32, DSPEED_HIP_NO_FUSED, ...): a plan stands for the program
// AND these, so whoever keeps planned chains by their program (dsp_gufuncs.cpp) keys on it as well
uint64_t dsp_plan_switches();
