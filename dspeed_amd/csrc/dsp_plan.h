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

// The argument blocks of the kernel-only routes (dsp_program.h): plain data, and of one plan exactly one is live
union KernelOnlyArgs {
    const void* wf;  // (every block begins with its rows)
    ExtremaArgs ext;
    HistArgs hist;
    ThreshArgs thresh;
    SpectrumArgs spec;
    SortArgs sort;
    InterpArgs interp;
    DenseArgs dense;
    ReflectArgs reflect;
    PileupArgs pileup;
    PulsesArgs pulses;
    TailfitArgs tailfit;
    AlignArgs align;
    SvmArgs svm;
};
static_assert(offsetof(ExtremaArgs, wf) == 0 && offsetof(HistArgs, wf) == 0 && offsetof(ThreshArgs, wf) == 0 && offsetof(SpectrumArgs, wf) == 0 &&
                  offsetof(SortArgs, wf) == 0 && offsetof(InterpArgs, wf) == 0 && offsetof(DenseArgs, wf) == 0 && offsetof(ReflectArgs, wf) == 0 &&
                  offsetof(PileupArgs, wf) == 0 && offsetof(PulsesArgs, wf) == 0 && offsetof(TailfitArgs, wf) == 0 && offsetof(AlignArgs, wf) == 0 &&
                  offsetof(SvmArgs, wf) == 0,
              "wf of KernelOnlyArgs");
// "the pointer at byte `at` of the live block is binding `io`": its first element, io_ptrs[io] + offset -- or, raw, io_ptrs[io] as it is
// handed in, for the inputs whose offset travels in the arguments
struct KernelBinding {
    int32_t io;  // (negative, as an op names an operand it does not have: the pointer stays null)
    uint16_t at;
    bool raw;
};
constexpr int DSP_KERNEL_BINDINGS_MAX = 14;  // (the pile-up kernel takes 10)
constexpr int DSP_KERNEL_ONLY_ROUTES = DSP_ROUTE_SCALAR;  // DSP_ROUTE_EXTREMA .. DSP_ROUTE_SVM: the routes ahead of the optimisations

struct ChainPlan;
// (dsp_plan.cpp; exported for the CPU tests)
extern "C" void dsp_internal_plan_energy_carries(int Ci, int S, const int32_t* lags, EnergyPlan* plan);
// What a launch of a kernel-only chain hands its kernel: the plan's block with the pointers of this call, every one from the list of
// bindings, and the flag of the 16-byte stores.  No HIP: tests/*_plan_fuzz.cpp call it with addresses nobody dereferences.
extern "C" void dsp_internal_plan_fill_args(const ChainPlan* ch, void* const* io_ptrs, KernelOnlyArgs* args);

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
    // The ops no interpreter case stands behind: a program that holds one runs on that op's kernel or is refused (kernel_only_routes,
    // dsp_plan.cpp: a row per route).  A program never matches two, so one argument block, one row source and one list of bindings serve them
    // all; DSP_ROUTE_VM: the program holds no such op and none of the four means anything.
    dsp_route kernel_only = DSP_ROUTE_VM;
    KernelOnlyArgs only{};  // the block of `kernel_only`, its pointers null (dsp_internal_plan_fill_args fills them per call)
    RowSource only_src{};   // (io < 0: histogram_stats alone, on weights and edges read from rows; dtype then the loop's)
    KernelBinding bound[DSP_KERNEL_BINDINGS_MAX]{};
    int n_bound = 0;
    // the 16-byte stores of the kernels that have them: the int32 flag at out_vec_at of the block is set per call where the pointer at
    // out_ptr_at is aligned and not null.  -1: none -- the route has no such stores, the output's stride is no whole number of vectors, or
    // (dsp_align.hip) the launch starts with the op that streams nothing out
    int out_vec_at = -1, out_ptr_at = -1;
    // the binding recorded for a pointer of `only` (c.bound_io(c.only.sort.out)), or -1: the pointer stays null
    template <typename T>
    int bound_io(T* const& member) const {
        const size_t at = (size_t)((const char*)&member - (const char*)&only);
        for (int k = 0; k < n_bound && k < DSP_KERNEL_BINDINGS_MAX; ++k)  // (n_bound counts past the capacity: the overflow dsp_plan_build refuses)
            if (bound[k].at == at) return bound[k].io;
        return -1;
    }
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
// what is HIP-free about the launch of a kernel-only chain (kernel_only_routes): the dynamic LDS its kernel's limit is raised to at chain
// creation (0: the route has no limit to raise), and what dsp_chain_geometry reports
int dsp_plan_kernel_only_lds(const ChainPlan* ch);
void dsp_plan_kernel_only_geometry(const ChainPlan* ch, int64_t n_wf, int* lds_bytes_per_wave, int* waves_per_block, int* blocks);
// a digest of every environment switch dsp_plan_build reads (DSPEED_HIP_FIR_F32, DSPEED_HIP_NO_FUSED, ...): a plan stands for the program
// AND these, so whoever keeps planned chains by their program (dsp_gufuncs.cpp) keys on it as well
uint64_t dsp_plan_switches();
