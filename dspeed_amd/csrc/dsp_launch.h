// dsp_launch.h -- the launchers the .hip files define for dsp_host.cpp (and for each other), each declared here and nowhere else.  Every
// file that defines one includes this header, so a definition that disagrees with what its caller sees does not compile (with C linkage it
// would link).  They return a hipError_t as int; dsp_internal_set_*_lds raises a kernel's dynamic-LDS limit.  Internal header.
#pragma once
#include <hip/hip_runtime.h>

#include "dsp_program.h"

extern "C" {
// dsp_vm.hip
int dsp_internal_launch_vm_f32(const DevProgram* dev_prog, const IoPtrs* ptrs, int64_t n_wf, int* err, int blocks, int threads, int lds_bytes,
                               int with_fir, int team, hipStream_t stream);
int dsp_internal_launch_vm_f64(const DevProgram* dev_prog, const IoPtrs* ptrs, int64_t n_wf, int* err, int blocks, int threads, int lds_bytes,
                               int with_fir, hipStream_t stream);
int dsp_internal_set_vm_lds(int lds_bytes);
int dsp_internal_launch_stream_read(const void* src, int64_t bytes, uint32_t* sink, int blocks, hipStream_t stream);
int dsp_internal_launch_synth(void* wf, int out_dtype, int64_t n_wf, int wf_len, int64_t row_stride, float* baseline, float* t_pick, uint64_t seed,
                              int64_t first_row, float tau, float sigma, float pick_offset, float bl_lo, float bl_hi, float amp_lo, float amp_hi,
                              float rise_lo, float rise_hi, hipStream_t stream);
// dsp_fit.hip
int dsp_internal_launch_fit_rows(const FitArgs* A, int wf_dtype, int compute_dtype, hipStream_t stream);
// dsp_energy.hip (npf: 16-byte loads per lane that cover a waveform; S: replay sub-chains, plan[S - 1]) and its second unit dsp_energy_h.hip
int dsp_internal_launch_energy(const EnergyArgs* A, int trap_opcode, int npf, int64_t n_wf, int* err, int blocks, int threads, int lds_bytes,
                               hipStream_t stream);
int dsp_internal_set_energy_lds(int trap_opcode, int npf, int lds_bytes);
int dsp_internal_launch_energy_rr(const EnergyArgs* A, const EnergyPlan* PL, int trap_opcode, int npf, int S, int wf_dtype, int64_t n_wf, int* err,
                                  int blocks, int threads, int lds_bytes, hipStream_t stream);
int dsp_internal_launch_energy_rr_h(const EnergyArgs* A, const EnergyPlan* PL, int trap_opcode, int npf, int S, int wf_dtype, int64_t n_wf, int* err,
                                    int blocks, int threads, int lds_bytes, hipStream_t stream);
// dsp_rows.hip, dsp_pz.hip, dsp_reduce.hip
int dsp_internal_launch_rows(const RowsArgs* A, int64_t n_wf, int* err, int lds_bytes, hipStream_t stream);
int dsp_internal_set_rows_lds(int lds_bytes);
int dsp_internal_launch_pz_rows(const PzArgs* A, int64_t n_wf, int* err, hipStream_t stream);
int dsp_internal_launch_reduce(const ReduceArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream);
// dsp_extrema.hip (dtype: the rows'; vec: rows start on 16-byte boundaries and hold whole 16-byte vectors)
int dsp_internal_launch_extrema(const ExtremaArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream);
// dsp_hist.hip (A->wf null: histogram_stats alone, dtype then the loop's type; LDS: dsp_hist::lds_bytes(A->m), below the 64 KiB that need no opt-in)
int dsp_internal_launch_hist(const HistArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream);
// dsp_thresh.hip (dtype: the rows'; vec as above; A->m 0: time_over_threshold, else multi_time_point_thresh with m thresholds)
int dsp_internal_launch_thresh(const ThreshArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream);
// dsp_spectrum.hip (dtype: the rows'; vec as above; the tables of A are the chain's; LDS: dsp_spectrum::lds_bytes, 16 bytes past 64 KiB for the longest rows)
int dsp_internal_launch_spectrum(const SpectrumArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream);
int dsp_internal_set_spectrum_lds(int dtype, int lds_bytes);
// dsp_sort.hip (dtype: the rows'; vec as above; LDS: dsp_sort::lds_bytes, 16 bytes past 64 KiB for the longest rows)
int dsp_internal_launch_sort(const SortArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream);
int dsp_internal_set_sort_lds(int dtype, int lds_bytes);
// dsp_interp.hip (dtype: the rows'; vec as above, for the loads -- the stores' is A->out_vec; LDS: dsp_interp::lds_bytes, 16 bytes past 64 KiB for the longest rows)
int dsp_internal_launch_interp(const InterpArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream);
int dsp_internal_set_interp_lds(int dtype, int lds_bytes);
// dsp_dense.hip (dtype: the rows'; vec as above; LDS: dsp_dense::lds_bytes, past 64 KiB for the widest layers)
int dsp_internal_launch_dense(const DenseArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream);
int dsp_internal_set_dense_lds(int dtype, int lds_bytes);
// dsp_reflect.hip (dtype: the rows'; vec as above, for the loads -- the stores' is A->out_vec; LDS: dsp_reflect::lds_bytes, up to 32 bytes past 64 KiB for the longest rows)
int dsp_internal_launch_reflect(const ReflectArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream);
int dsp_internal_set_reflect_lds(int dtype, int lds_bytes);
// dsp_pileup.hip (dtype: the rows'; vec as above, for the loads -- the stores' is A->out_vec; LDS: dsp_pileup::lds_bytes, static)
int dsp_internal_launch_pileup(const PileupArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream);
// dsp_pulses.hip (dtype: the rows'; vec as above, for the streaming pass of multi_a_filter; A->pick / A->amp: which of the two run)
int dsp_internal_launch_pulses(const PulsesArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream);
// dsp_tailfit.hip (dtype: the rows'; vec as above, for the loads -- the stores' is A->out_vec; LDS: dsp_tailfit::lds_bytes, static)
int dsp_internal_launch_tailfit(const TailfitArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream);
// dsp_align.hip (dtype: the rows'; the loop is A->f64; vec as above, for the streaming loads -- the stores' is A->out_vec; nothing in LDS)
int dsp_internal_launch_align(const AlignArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream);
// dsp_svm.hip (dtype: the rows'; the loop is A->f64; vec as above; LDS: dsp_svm::lds_bytes, past 64 KiB for resident rows of more than 64 samples and for more than 112 pairs)
int dsp_internal_launch_svm(const SvmArgs* A, int64_t n_wf, int dtype, int vec, int* err, hipStream_t stream);
int dsp_internal_set_svm_lds(int dtype, int f64, int lds_bytes);  // (called with dsp_svm::LDS_MAX: one value for every chain of a row type)
// dsp_scalar.hip (type: 0 float32, 1 float64, 2 int64 registers)
int dsp_internal_launch_scalar(const DevProgram* dev_prog, const IoPtrs* ptrs, int64_t n_wf, int n_sregs, int type, hipStream_t stream);
int dsp_internal_set_scalar_lds(int lds_bytes);
// dsp_current.hip, dsp_fir_runs.hip
int dsp_internal_launch_current(const CurrentArgs* A, int64_t n_wf, int blocks, int lds_bytes, hipStream_t stream);
int dsp_internal_set_current_lds(int lds_bytes);
int dsp_internal_launch_fir_runs(const FirRunsArgs* A, FirRunsTable* table, int64_t n_wf, int blocks, int* err, hipStream_t stream);
// dsp_fir_mfma.hip (dsp_internal_fir_fixup: the rows-with-a-NaN-or-an-infinity pass alone, also behind the float16 kept-output form)
int dsp_internal_launch_fir_mfma(const FirArgs* A, int64_t n_wf, int lds_bytes, hipStream_t stream);
int dsp_internal_set_fir_mfma_lds(int lds_bytes);
int dsp_internal_launch_fir_store(const FirArgs* A, int64_t n_wf, int lds_bytes, hipStream_t stream);
int dsp_internal_set_fir_store_lds(int lds_bytes);
int dsp_internal_fir_fixup(const FirArgs* A, int64_t n_wf, hipStream_t stream);
// dsp_fir_f16.hip
int dsp_internal_launch_fir_f16(const FirArgs* A, const FirF16Taps* T, int64_t n_wf, int lds_bytes, hipStream_t stream);
int dsp_internal_set_fir_f16_lds(int lds_bytes);
}
