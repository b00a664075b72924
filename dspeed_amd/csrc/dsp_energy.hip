// dsp_energy.hip -- the Ge energy chain as ONE specialised kernel (BASELINE.json configs[1]/[3]):
//
//     waveform --bl_subtract--> --pole_zero--> --trap_filter|trap_norm|asym_trap--> fixed_time_pickoff --> 1 float
//
// Same arithmetic as the generic waveform VM (dsp_vm.hip) -- the host selects these kernels when a chain has exactly this
// shape.  One wavefront per waveform, lane j owns a chunk of consecutive samples, the next waveform's 16 KB are already in
// flight (16-byte global loads into registers) while the current one is filtered, and the trapezoid output is never stored
// (only the picked-off samples are kept).  Two kernels:
//   * dsp_energy_rr_kernel ("register resident", the default for 1024 .. 8192 samples): pad-free LDS image (sample i at
//     element i, C = len/64 + 2 samples per lane: an even lane stride, so every lane's chunk starts 8-byte aligned and
//     "offsets t, t + 1 of my chunk" is one conflict-free 8-byte access), every pass over the chunk fully unrolled (immediate
//     LDS offsets, counted waits), the lane's own chunk in VGPRs from the staging to the end of the replay.  Per sample the
//     LDS sees 2 writes (staging, pole-zero output) and 4 reads (own chunk once, three lagged trapezoid streams), the reads
//     and the pole-zero output 8 bytes a lane at a time.
//     Built twice: for the two-point pick-off modes here, for the 4-point mode in dsp_energy_h.hip (this file again, as a second unit).
//   * dsp_energy_kernel ("classic"): the VM's slot layout (C = len/64, pitch C + 1, zero guard of 2 pitches below the slot),
//     chunk loops software-pipelined in groups of 8 samples.  Bit-identical to the VM; kept as the cross-check of the
//     default kernel and for A/B measurements (set_fused(15)).
// Reference bodies: processors/bl_subtract.py:11-46, pole_zero.py:24-77, trap_filters.py:12-227, fixed_time_pickoff.py:12-125.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "dsp_kernels.h"
#include "dsp_launch.h"
#include "dsp_wave.h"

#ifdef DSPEED_HIP_DIAG
#define ABLATE(A) ((A).ablate)
#else
#define ABLATE(A) 0
#endif

// Wave priority by phase (s_setprio).  Two wavefronts share a SIMD, and each issues at most one instruction per four cycles: what the
// kernel gains from the second one is the overlap of one wavefront's dependent chains (pass 2's float64 recurrence, the scans and lane
// exchanges of the carries, the four-addition replay of pass 3, the tail) with the other's bulk work (staging stores, the chunk load,
// the float64 sums of pass 1).  The hardware arbitrates by priority, then age; with equal priorities the OLDER wavefront wins whatever
// it is doing, and a wavefront in a dependent chain loses its slot to the other's independent instructions every other time.  Priority
// that rises with the phase -- stage 0, pass 1 at 1, pass 2 at 2, carries / replay / tail at 3 -- lets the chain that is closest to
// finishing a row issue whenever it can and fills the gaps with the younger row's bulk work: 62.8 % -> 68.9 % of the HBM peak on the same
// box, same instructions (profiles/r03_headline_experiments.md: 20 sequences measured, every graded one within 0.5 % of this).
constexpr int rr_prio_after_phase[6] = {1, 2, 3, 3, 3, 0};  // priority of the phase that FOLLOWS boundary n (5: the next row's staging)
#define RR_PRIO_AT(n) __builtin_amdgcn_s_setprio(rr_prio_after_phase[n]);

// Two 8-byte LDS accesses of one lane are otherwise merged into one ds_read2_b64 / ds_write2_b64, which the LDS serves at the rate of the
// 4-byte forms (8 array cycles for 16 bytes a lane; ds_read_b64: 2 cycles for 8).  An instruction with side effects between them, itself
// nothing, ends the merge.  The "memory" clobber is a full compiler barrier for memory: besides ending the merge it keeps every LDS and
// global access, related or not, on its side of the macro (about 150 places per row, all inside passes that are ordered by their data
// anyway; the prefetch and the result store sit between sched_barriers of their own).  It emits no instruction and no wait.  The build
// counts the fused forms in the rr kernels' code and fails if any appear (RR_NO_FUSED_LDS in build.py).
#define RR_NO_MERGE() asm volatile("" ::: "memory")

namespace {

constexpr int G = 8;   // samples per software-pipeline group in the pole-zero passes
constexpr int G3 = 8;  // ... in the trapezoid replay (4 streams x 2 buffers live there: 64 VGPRs, fine at 2 waves/SIMD)

// diagnostic cycle stamps (DSPEED_HIP_ABLATE bit 3): where a wavefront spends its time, summed per phase into err[4 + 2*phase]
__device__ __forceinline__ unsigned long long stamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define PHASE(i)                                   \
    if (stamps) {                                  \
        const unsigned long long now_ = stamp();   \
        tsum[i] += now_ - tlast;                   \
        tlast = now_;                              \
    }

// first pair that stage st of the replay loads of a lagged stream with parity par (dsp_energy_rr_kernel), np = pairs the sub-chain needs
constexpr int rr_pair_lo(int st, int par, int np) { return st == 0 ? 0 : (2 * st + par < np ? 2 * st + par : np); }

template <int N>
__device__ __forceinline__ void load_group(float (&v)[N], const float* p) {
#pragma unroll
    for (int u = 0; u < N; ++u) v[u] = p[u];
}

template <int NPF, int KIND>
__global__ void __launch_bounds__(256, 2) dsp_energy_kernel(EnergyArgs A, int64_t n_wf, int* err) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = lane_id();
    const double inv_rr = 1.0 / A.rr, inv_ll = 1.0 / A.ll;  // trap_norm / asym_trap divide by these counts every sample
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), wpb = (int)(blockDim.x >> 6);  // provably wave-uniform
    float* lds = reinterpret_cast<float*>(smem_raw) + (size_t)wave * A.lds_elems_per_wave;
    for (int e = lane; e < A.lds_elems_per_wave; e += 64) lds[e] = 0.0f;
    wave_sync();

    // the host selects this kernel only for len == 256 * NPF: every lane owns exactly C = 4 * NPF samples, no tail
    constexpr int C = 4 * NPF, pitch = C + 1, len = 256 * NPF;
    float* slot = lds + A.slot_off;
    float* mine = slot + lane * pitch;

    // lagged-read bases (identical for every row): see trap_core in dsp_vm.hip
    const float* lagp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int jj = lane - A.q[k] - 1;
        lagp[k] = (jj >= -1) ? slot + jj * pitch + (C - A.rho[k]) : slot - 2 * pitch;
    }

    const int64_t stride_rows = (int64_t)gridDim.x * wpb;
    int64_t row = (int64_t)blockIdx.x * wpb + wave;

    typedef float f4 __attribute__((ext_vector_type(4)));
    f4 pf[NPF];
    float pf_bl = 0.0f, pf_tp = 0.0f;
    auto prefetch = [&](int64_t r) {
        const float* g = (const float*)A.wf + r * A.wf_stride + A.wf_offset;
#pragma unroll
        for (int b = 0; b < NPF; ++b) pf[b] = reinterpret_cast<const f4*>(g)[b * 64 + lane];
        pf_bl = A.bl ? A.bl[r * A.bl_stride] : A.bl_const;  // 0 when the chain has no bl_subtract: x - 0 == x exactly
        pf_tp = A.tp ? A.tp[r * A.tp_stride] : A.tp_const;
    };
    auto report = [&](int code, int64_t r) {
        if (lane == 0 && atomicCAS(&err[0], 0, code) == 0) {
            err[1] = (int)(r & 0xffffffffll);
            err[2] = (int)(r >> 32);
        }
    };
    if (row < n_wf) prefetch(row);
    const bool stamps = (ABLATE(A) & 8) != 0;
    unsigned long long tsum[6] = {0, 0, 0, 0, 0, 0}, tlast = stamps ? stamp() : 0;

    for (; row < n_wf; row += stride_rows) {
        // ---- stage the prefetched waveform into LDS (chunked layout)
#pragma unroll
        for (int b = 0; b < NPF; ++b) {
            const int e = (b * 64 + lane) * 4;
            float* d = slot + e + e / C;  // sample e -> element e + e / C (chunk pad)
#pragma unroll
            for (int m = 0; m < 4; ++m) d[m] = pf[b][m];
        }
        // per-waveform scalars are wave-uniform: say so, or every use downstream becomes per-lane (exec-masked) code
        const float bl = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(pf_bl)));
        const float t_in = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(pf_tp)));
        const int64_t next = row + stride_rows;
        __builtin_amdgcn_sched_barrier(0);  // the staging stores must issue before the registers are reloaded
        if (next < n_wf) prefetch(next);    // in flight while this waveform is filtered
        __builtin_amdgcn_sched_barrier(0);
        wave_sync();
        PHASE(0)

        float result = quiet_nan<float>();
        // ---- pass 1: per-chunk float64 sum of x = w - baseline; a NaN anywhere (or a NaN baseline) poisons the sum
        double X = 0.0;
        if (!(ABLATE(A) & 1)) {
            float va[G], vb[G];
            load_group(va, mine);
#pragma unroll 1
            for (int t = 0; t < C; t += 2 * G) {
                load_group(vb, mine + t + G);
#pragma unroll
                for (int u = 0; u < G; ++u) X += (double)(va[u] - bl);
                if (t + 2 * G < C) load_group(va, mine + t + 2 * G);
#pragma unroll
                for (int u = 0; u < G; ++u) X += (double)(vb[u] - bl);
            }
        }
        bool in_nan = A.tau_nan != 0;
        if (wave_any(!(fabs(X) <= 1.7976931348623157e308))) {
            // NaN or infinite sum: look for real NaNs (an infinite input is not NaN for the reference, pole_zero.py:55-58)
            bool n = false;
            for (int t = 0; t < C; ++t) {
                const float x = mine[t] - bl;
                n |= (x != x);
            }
            in_nan |= wave_any(n);
        }
        PHASE(1)
        if (!in_nan) {
            const double E = wave_exscan_add(X);
            const float xlast = mine[C - 1] - bl;
            const double xprev0 = (double)wave_prev(xlast);
            // ---- pass 2: pole-zero recurrence in the reference's operation order, output in place; float32 running sum of
            // the output feeds the speculative carries of the trapezoid
            const double c = A.c;
            double acc = E - c * (E - xprev0), xp = xprev0;
            float run = 0.0f, cap[3] = {0.0f, 0.0f, 0.0f};
            if (!(ABLATE(A) & 2)) {
                float va[G], vb[G];
                load_group(va, mine);
                auto body = [&](float (&v)[G], int t) {
                    float rs[G];
#pragma unroll
                    for (int u = 0; u < G; ++u) {
                        const double x = (double)(v[u] - bl);
                        acc = (acc + x) - xp * c;
                        const float y = (float)acc;
                        mine[t + u] = y;
                        xp = x;
                        run += y;
                        rs[u] = run;
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const int d = ((C - A.rho[k]) % C) - t;  // prefix needed by lag k completes after d samples of this group
                        if (d >= 1 && d <= G) {
#pragma unroll
                            for (int u = 0; u < G; ++u)
                                if (d == u + 1) cap[k] = rs[u];
                        }
                    }
                };
#pragma unroll 1
                for (int t = 0; t < C; t += 2 * G) {
                    load_group(vb, mine + t + G);
                    body(va, t);
                    if (t + 2 * G < C) load_group(va, mine + t + 2 * G);
                    body(vb, t + G);
                }
            }
            wave_sync();
            PHASE(2)
            bool pz_nan = false;
            if (wave_any(!(fabsf(run) <= 3.4028234663852886e38f))) {
                bool n = false;
                for (int t = 0; t < C; ++t) {
                    const float y = mine[t];
                    n |= (y != y);
                }
                pz_nan = wave_any(n);
            }
            if (pz_nan) {
                report(DSP_E_PZ_NAN, row);  // pole_zero.py:76-77
            } else if (!A.all_nan && !(ABLATE(A) & 4) && pickoff_in_range(t_in, len)) {
                // ---- speculative carries: filter value at every chunk boundary from the prefix sums
                const double Ep = wave_exscan_add((double)run);
                double Ak[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const bool whole = (A.rho[k] == 0);
                    Ak[k] = wave_shift_up(Ep + (whole ? 0.0 : (double)cap[k]), A.q[k] + (whole ? 0 : 1));
                }
                double Gd;
                if (KIND == TRAP_FILTER)
                    Gd = ((Ep - Ak[0]) - Ak[1]) + Ak[2];
                else if (KIND == TRAP_NORM)
                    Gd = (((Ep - Ak[0]) - Ak[1]) + Ak[2]) / A.rr;
                else
                    Gd = (Ep - Ak[0]) / A.rr - (Ak[1] - Ak[2]) / A.ll;
                const float g = (lane == 0) ? -0.0f : (float)Gd;

                // ---- pick-off positions (uniform): samples i0-1 .. i0+2, kept only where the mode needs them
                const int i0 = (int)t_in;
                const bool wide = (A.mode == 'h');
                int cl[4], co[4];
                float capv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = i0 - 1 + k;
                    const bool need = ((k == 1) || (k == 2) || wide) && e >= 0 && e < len;
                    const int l = need ? e / C : -1;
                    cl[k] = l;
                    co[k] = need ? e - l * C : -1000;
                    capv[k] = 0.0f;
                }
                // groups of the replay loop that contain a wanted sample (uniform bit mask)
                unsigned capmask = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (co[k] >= 0) capmask |= 1u << (co[k] / G3);
                PHASE(3)
                // ---- pass 3: replay the reference's float32 rounding sequence over the chunk
                float y = g;
                {
                    float a0[G3], a1[G3], a2[G3], a3[G3], b0[G3], b1[G3], b2[G3], b3[G3];
                    auto fetch = [&](float (&o)[G3], float (&l0)[G3], float (&l1)[G3], float (&l2)[G3], int t) {
                        load_group(o, mine + t);
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            float(&dst)[G3] = (k == 0) ? l0 : (k == 1 ? l1 : l2);
                            const int r = A.rho[k];
                            if (t >= r) {
                                load_group(dst, lagp[k] + t + 1);
                            } else if (t + G3 <= r) {
                                load_group(dst, lagp[k] + t);
                            } else {
#pragma unroll
                                for (int u = 0; u < G3; ++u) dst[u] = lagp[k][t + u + ((t + u >= r) ? 1 : 0)];
                            }
                        }
                    };
                    auto body = [&](float (&o)[G3], float (&l0)[G3], float (&l1)[G3], float (&l2)[G3], int t) {
                        float ys[G3];
#pragma unroll
                        for (int u = 0; u < G3; ++u) {
                            y = trap_step_r<float, KIND>(y, o[u], l0[u], l1[u], l2[u], A.rr, A.ll, inv_rr, inv_ll);
                            ys[u] = y;
                        }
                        if ((capmask >> (t / G3)) & 1u) {
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                const int d = co[k] - t;
#pragma unroll
                                for (int u = 0; u < G3; ++u)
                                    if (d == u) capv[k] = ys[u];
                            }
                        }
                    };
                    fetch(a0, a1, a2, a3, 0);
#pragma unroll 1
                    for (int t = 0; t < C; t += 2 * G3) {
                        fetch(b0, b1, b2, b3, t + G3);
                        body(a0, a1, a2, a3, t);
                        if (t + 2 * G3 < C) fetch(a0, a1, a2, a3, t + 2 * G3);
                        body(b0, b1, b2, b3, t + G3);
                    }
                }
                PHASE(4)
                // ---- true carries from the per-chunk increments (exact scan), then the pick-off
                const double D = (double)y - (double)g;
                const double delta = wave_exscan_add(D) - (double)g;
                float w4[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float v = (float)((double)capv[k] + delta);
                    w4[k] = cl[k] >= 0 ? readlane(v, cl[k]) : 0.0f;
                }
                int fc = 0;
                result = pickoff_eval(t_in, A.mode, len, w4, fc);
                if (fc) report(fc, row);
            }
        }
        if (lane == 0) A.out[row * A.out_stride] = result;
        wave_sync();
        PHASE(5)
    }
    if (stamps && lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) atomicAdd(reinterpret_cast<unsigned long long*>(err + 4) + i, tsum[i]);
    }
}

// ------------------------------------------------------------------------------------------------
// "rr" (register resident) kernel.
//
// What the measurements on MI355X said (profiles/r01_summary.md has the counters): a wavefront of this chain is bound by its
// own instruction stream -- about one instruction per 4 cycles, an LDS access several times that -- and at 17-20 KB of LDS
// per waveform only 2 wavefronts fit a SIMD, so nothing hides a stall.  Hence:
//   * every pass over the C samples of a lane is straight-line code (no loop counters, no address arithmetic, no uniform
//     branches inside: with those hipcc falls back to s_waitcnt lgkmcnt(0) and serialises LDS latency with the arithmetic);
//   * the chunk is read from LDS once and stays in VGPRs through pass 1 (float64 sum), pass 2 (pole-zero, in place) and
//     pass 3 (trapezoid replay); only the three lagged streams of the replay come from LDS, loaded PD stages ahead;
//   * bl_subtract happens in the staging stores; the result of row r is stored behind the prefetch of row r + 2 (vmcnt
//     counts stores: a store at the end of the loop body would sit in front of the next staging's s_waitcnt vmcnt(0));
//     the row loads are non-temporal (a launch streams every byte once, past every cache: + 1.8 % alone), and in the build for
//     4096-sample float32 rows they are issued behind pass 2, which lends their registers to 32 float64 images that pass 2 then
//     does not convert again (KD below).  The sample in front of a lane's chunk comes from the lane below by DPP, not from LDS;
//     the replay's group-start states are stored by the 4-point build alone, which is the one that reads them; lanes whose lagged
//     window lies wholly below sample 0 read the guard at addresses of their own banks.  Figures: profiles/r07_headline_trims.md.
//   * what must be picked out at a run-time position is never tested per sample, and where the position is wave-uniform and the
//     values are the lane's own registers it does not go through LDS either: the float32 prefix sums at the 8-sample group ends are a
//     register vector that the carries index (s_set_gpr_idx_on, one v_mov_b32); the two trapezoid samples every pick-off mode needs
//     are indexed out of a 16-sample register window under one uniform branch per 16 samples (a not-taken branch costs tens of
//     cycles; 32 of them cost more than they saved), by every lane -- the tail's readlane names the owner.  The replay state at each
//     group start goes to a 9-entry per-lane LDS side array in the 4-point build, which re-runs a group from it (a run-time group
//     number is then an address for the samples too).  The carries' capture groups are still read from LDS: xr is 66 registers, an
//     indexed move reaches 32, and two uniform branches and eight indexed moves a lag cost more than the 12 pipelined reads
//     they replace (built and measured: 3 % slower).  Figures: profiles/r10_headline_register_picks.md.
//   * the LDS array serves a ds_read_b64 in 2 cycles and a ds_read2_b32 -- the same 8 bytes a lane -- in 4, and the array was busy
//     two thirds of the kernel's time.  So the lane pitch is even, C = len/64 + 2: every lane's chunk starts 8-byte aligned, the
//     chunk is NG = (C - 2) / 8 groups of 8 samples and a two-sample tail (the tail extends the last replay chain; where the
//     passes speak of "group NG" they mean it), the 64 C - len = 128 virtual samples above len are cleared with every staging,
//     and lanes past (len - 1) / C filter zeros.  The own chunk is read as C / 2 pairs, pass 2 stores its output as pairs (4-byte
//     stores at an even pitch put two lanes on one bank), the capture reads are pairs.  A lagged window starts at element
//     lane C - lag: aligned when the lag is even; when it is odd the aligned pairs start one element lower and step t takes
//     element t + 1 of them.  Which register that is, is a compile-time matter once the lag's parity is: the replay is a generic
//     lambda over the three parities, instantiated per case (4 for trap_filter / trap_norm, whose third lag 2 rise + flat has the
//     parity of the other two's sum; 8 for asym_trap) and selected by one wave-uniform switch per row -- a wavefront runs one copy for
//     the whole launch.  The compiler would fuse neighbouring 8-byte accesses into ds_read2_b64 / ds_write2_b64, which the LDS
//     serves at the 4-byte rate again: RR_NO_MERGE keeps them apart.  The 8-sample re-run of the 4-point pick-off mode reads
//     4 bytes at a run-time position and needs no parity case.  Figures: profiles/r05_headline_lds.md.
//   * a wavefront issues at most one instruction per four cycles and the kernel's two wavefronts per SIMD saturate no pipe: outside the
//     sample passes every instruction, scalar ones included, costs its four cycles, a branch tens.  So what a row does not need to work
//     out is not worked out per row.  The carries take their plan from the host as it is used (EnergyPlan: pair address, side
//     element, count; a capture in group 0 picks an element that holds 0.0f instead of selecting), held as lane addresses and one packed
//     scalar across the row loop, and sum "the first pn of 8 samples" as all eight running prefixes and one indexed register move
//     (s_set_gpr_idx_on with the wave-uniform pn) instead of eight masked additions.  The pick-off mode is a build of the kernel
//     (WIDE): the two-point modes n f c l i end in straight-line selects, and only the build for the 4-point mode h holds the two
//     8-sample re-runs.  Figures: profiles/r06_headline_serial.md.
// S = sub-chains of the replay per lane: 2 halves the dependent-add chain but doubles the carry captures; measured slower.
// ------------------------------------------------------------------------------------------------
// IN: waveform element type in HBM: 0 float32, 1 int16, 2 uint16 (digitiser samples; widened to float32 while staging, exactly
// like the reference's ufunc casting picks the float32 loop for them, processing_chain.py:1565-1572)
// exp(-1 / tau) in float64 for a time constant that varies per event, as the interpreter's op forms it (dsp_vm.hip pz_decay; pole_zero.py:60):
// out of line, the device's exp is 200 instructions
__device__ __attribute__((noinline)) double rr_decay(double tau) { return exp(-1.0 / tau); }

template <int NPF, int KIND, int S, int IN, bool TAU, bool WIDE>
__global__ void __launch_bounds__(256, NPF >= 32 ? 1 : 2) dsp_energy_rr_kernel(EnergyArgs A, EnergyPlan PL, int64_t n_wf, int* err) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    // a chunk = NG groups of 8 samples (S sub-chains of NGS groups) and a two-sample tail that extends the last sub-chain
    constexpr int C = 4 * NPF + 2, len = 256 * NPF, NG = (C - 2) / 8, CS = (C - 2) / S, NGS = CS / 8;
    constexpr int BS = CS >= 16 ? 16 : CS;  // samples per capture block
    static_assert((C - 2) % (8 * S) == 0, "sub-chain length must be a whole number of 8-sample groups");
    static_assert(C % 2 == 0 && 64 * C - len == 128, "even pitch: 8-byte aligned lane chunks, two rows of virtual samples above len");
    typedef float f2 __attribute__((ext_vector_type(2)));
    typedef float f9 __attribute__((ext_vector_type(9)));
    const int lane = lane_id();
    const double inv_rr = 1.0 / A.rr, inv_ll = 1.0 / A.ll;  // trap_norm / asym_trap divide by these counts every sample
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), wpb = (int)(blockDim.x >> 6);
    float* lds = reinterpret_cast<float*>(smem_raw) + (size_t)wave * A.lds_elems_per_wave;
    for (int e = lane; e < A.lds_elems_per_wave; e += 64) lds[e] = 0.0f;
    wave_sync();
    float* slot = lds + A.slot_off;
    float* mine = slot + lane * C;
    f2* mine2 = reinterpret_cast<f2*>(mine);  // (the wave's region, slot_off and lane * C are all even numbers of elements)
    // per-lane side array (pitch 9, odd): the group-start states of the replay, which the 4-point build alone stores and reads.  Kept in
    // LDS so that "the state of group gi" with a run-time gi is an address, and its eight-sample re-run reads samples at one too
    // (9 for up to 4096 samples, 17 for 8192).  The group-end prefix sums of pass 2 lived here once; they stay in registers now, and so do
    // the two pick-off samples, whose 2 x 16-float capture buffer above the side arrays is still part of the layout, unused.
    // The region's layout is the planner's, which sizes it and sets slot_off: dsp_kernels.h
    constexpr int AUXP = dsp_energy_rr::layout(C).side_pitch, GUARD = dsp_energy_rr::layout(C).guard, TAIL = dsp_energy_rr::layout(C).tail;
    static_assert(NG + 1 <= AUXP && S * NGS + 1 <= AUXP && (AUXP & 1) == 1, "side array too small");
    static_assert(GUARD >= 2 * C + 8 && GUARD >= C + 64 + dsp_energy_rr::WINDOW_SPAN_EXTRA && dsp_energy_rr::layout(C).slot_off >= GUARD,
                  "lagged reads before sample 0 stay inside the guard");
    float* aux = slot + 64 * C + TAIL + lane * AUXP;
    // the lagged window of the lane starts at element lane*C - lag: 8-byte aligned for an even lag; for an odd one the aligned pairs
    // start one element lower and step t takes element t + 1 of them.  lagb[] is that aligned start, lagpar[] the wave-uniform,
    // row-invariant parity of each lag.  A window wholly below sample 0 reads zeros of the guard, at the guard address that equals its
    // natural one modulo 64 elements (dsp_kernels.h: one address for all such lanes shares a bank pair with a lane that reads the image,
    // in every access of the replay -- 68 conflict cycles a row at the benchmark's lags)
    const float* lagb[3];
    int lagpar[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lagpar[k] = A.q[k] & 1;                           // q[] carries the lags
        lagb[k] = slot + dsp_energy_rr::lag_window_start(C, GUARD, lane, A.q[k]);
    }
    // the carry plan (row-invariant): the capture group's pairs as an address of this lane ...
    const f2* capp[3][S];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int s = 0; s < S; ++s) capp[k][s] = mine2 + (PL.grp[k][s] >> 1);
    // ... and the three counts pn of a sub-chain and the three group-end sums in front of the capture groups in one scalar, opaque to the
    // optimiser: it is then one live register, not six words of the kernel's arguments loaded again in every row (the kernel is at its
    // scalar-register limit).  Bits 4 k .. 4 k + 3: pn of lag k; bits 12 + 5 k .. 16 + 5 k: 1 + the plan's side element, 0 = a capture in
    // group 0, nothing in front (element 0 of pass 2's vector of group-end sums holds 0.0f)
    float zero = 0.0f;  // P[0] of the prefixes, as a register (a constant element makes the compiler fill the vector from scalars first)
    asm volatile("" : "+v"(zero));
    static_assert(NG + 1 <= 32, "a side element and its + 1 fit 5 bits");
    int pnpack[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        pnpack[s] = PL.pn[0][s] | (PL.pn[1][s] << 4) | (PL.pn[2][s] << 8) | ((PL.side[0][s] + 1) << 12) | ((PL.side[1][s] + 1) << 17) |
                    ((PL.side[2][s] + 1) << 22);
        asm volatile("" : "+s"(pnpack[s]));
    }

    const int64_t stride_rows = (int64_t)gridDim.x * wpb;
    int64_t row = (int64_t)blockIdx.x * wpb + wave;
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    constexpr int NLD = IN == 0 ? NPF : NPF / 2;  // 16-byte loads per lane and waveform: 4 float32 or 8 16-bit samples each
    static_assert(IN == 0 || NPF % 2 == 0, "16-bit rows: an even number of 4-sample groups per lane");
    // Pass 2 needs the float64 image of every sample pass 1 has just formed; all C of them are 2 C registers the kernel does not have,
    // so pass 2 converts again.  The 4 NPF registers of the next row's prefetch are the largest block that can be had: where KD > 0 the
    // prefetch (and the pending result store with it) is issued behind pass 2 instead of behind the staging, the loads then have the
    // carries, pass 3 and the tail to arrive in (about half a row: enough, measured), and the first KD images of pass 1 are kept for
    // pass 2 -- the same conversions of the same values.  KD = 32 is the measured best of 16 / 24 / 32 for 4096-sample float32 rows
    // with one time constant (237 VGPRs, no scratch, no AGPR copies, two wavefronts per SIMD); the other builds keep the early prefetch.
    constexpr int KD = (NPF == 16 && S == 1 && IN == 0 && !TAU) ? 32 : 0;
    constexpr bool LATE = KD > 0;
    u4 pf[NLD];
    float pf_bl = 0.0f, pf_tp = 0.0f;
    auto prefetch = [&](int64_t r) {
        const char* g = (const char*)A.wf + (r * A.wf_stride + A.wf_offset) * (IN == 0 ? 4 : 2);
#pragma unroll
        for (int b = 0; b < NLD; ++b)  // (non-temporal: every byte of a row is read once per launch, and a launch's rows do not fit any cache)
            pf[b] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(g) + b * 64 + lane);
        // (address space 1 spelled out: a pointer that went through a null test is otherwise loaded with flat_load, whose
        // out-of-order return forces every LDS wait that follows it down to lgkmcnt(0))
        typedef const __attribute__((address_space(1))) float* gptr;
        pf_bl = A.bl ? ((gptr)A.bl)[r * A.bl_stride] : A.bl_const;
        pf_tp = A.tp ? ((gptr)A.tp)[r * A.tp_stride] : A.tp_const;
    };
    auto report = [&](int code, int64_t r) {
        if (lane == 0 && atomicCAS(&err[0], 0, code) == 0) {
            err[1] = (int)(r & 0xffffffffll);
            err[2] = (int)(r >> 32);
        }
    };
    if (row < n_wf) prefetch(row);
    const bool stamps = (ABLATE(A) & 8) != 0;
    unsigned long long tsum[6] = {0, 0, 0, 0, 0, 0}, tlast = stamps ? stamp() : 0;
    // a row's result is stored one iteration late, behind the next prefetch: vmcnt counts stores too, so a store issued
    // at the end of the loop body would sit (a full write latency) in front of the s_waitcnt vmcnt(0) that opens the next staging
    float pend_result = 0.0f;
    int64_t pend_row = -1;

    for (; row < n_wf; row += stride_rows) {
        // bl_subtract while staging (16-bit samples: unpacked and converted first; a lane's load covers 8 consecutive samples)
#pragma unroll
        for (int b = 0; b < NLD; ++b) {
            if (IN == 0) {
                f4 v;
#pragma unroll
                for (int m = 0; m < 4; ++m) v[m] = __uint_as_float(pf[b][m]);
                *reinterpret_cast<f4*>(slot + (b * 64 + lane) * 4) = v - pf_bl;
            } else {
                f4 lo, hi;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const unsigned int wv = pf[b][m];
                    const float s0 = IN == 1 ? (float)(short)(wv & 0xffffu) : (float)(wv & 0xffffu);
                    const float s1 = IN == 1 ? (float)(short)(wv >> 16) : (float)(wv >> 16);
                    if (m < 2) {
                        lo[2 * m] = s0;
                        lo[2 * m + 1] = s1;
                    } else {
                        hi[2 * (m - 2)] = s0;
                        hi[2 * (m - 2) + 1] = s1;
                    }
                }
                *reinterpret_cast<f4*>(slot + (b * 64 + lane) * 8) = lo - pf_bl;
                *reinterpret_cast<f4*>(slot + (b * 64 + lane) * 8 + 4) = hi - pf_bl;
            }
        }
        // the 64*C - len = 128 virtual samples above len, every row: pass 2 left the decaying pole-zero tail of the last row in them
        reinterpret_cast<f2*>(slot + len)[lane] = f2{0.0f, 0.0f};
        const float t_in = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(pf_tp)));
        const int64_t next = row + stride_rows;
        auto fetch_next = [&]() __attribute__((always_inline)) {
            __builtin_amdgcn_sched_barrier(0);
            if (next < n_wf) prefetch(next);
            if (pend_row >= 0 && lane == 0) A.out[pend_row * A.out_stride] = pend_result;
            __builtin_amdgcn_sched_barrier(0);
        };
        bool fetched = false;
        if constexpr (!LATE) fetch_next();
        wave_sync();
        PHASE(0)
        RR_PRIO_AT(0)

        float result = quiet_nan<float>();
        // ---- the lane's chunk lives in registers from here to the end of the replay: x, then (in place) the pole-zero output
        float xr[C];
#pragma unroll
        for (int j = 0; j < C / 2; ++j) {  // 8 bytes per lane and read: lane bases are 8-byte aligned at the even pitch
            const f2 v = mine2[j];
            RR_NO_MERGE();
            xr[2 * j] = v.x;
            xr[2 * j + 1] = v.y;
        }
        const float xprev = wave_prev(xr[C - 1]);  // the sample in front of the chunk is the lane below's last (lane 0: 0.0f)
        // ---- pass 1: float64 sum of x over the chunk
        // (four partial sums: the float64 sum of 66 float32 samples is exact for one waveform's dynamic range, so the order is free,
        // and one chain of dependent float64 adds would cost their full latency 66 times)
        double Xp[4] = {0.0, 0.0, 0.0, 0.0};
        double xd[KD > 0 ? KD : 1];
#pragma unroll
        for (int t = 0; t < C; ++t) {
            if ((t & 7) == 0) __builtin_amdgcn_sched_barrier(0);  // (keeps the float64 conversions from being hoisted: registers)
            if (t < KD) {
                xd[t] = (double)xr[t];
                Xp[t & 3] += xd[t];
            } else {
                Xp[t & 3] += (double)xr[t];
            }
        }
        const double X = (Xp[0] + Xp[1]) + (Xp[2] + Xp[3]);
        double c_row = A.c;
        bool in_nan = A.tau_nan != 0;
        if constexpr (TAU) {  // (a build of its own: the constant-tau kernels keep their code)
            const float tau = A.tau[row * A.tau_stride];
            in_nan = tau != tau;
            c_row = rr_decay((double)tau);
        }
        if (wave_any(!(fabs(X) <= 1.7976931348623157e308))) {
            bool n = false;
#pragma unroll
            for (int t = 0; t < C; ++t) n |= (xr[t] != xr[t]);
            in_nan |= wave_any(n);
        }
        PHASE(1)
        RR_PRIO_AT(1)
        // the float64 images of the samples past the first KD are cheaper to recompute in pass 2 than to keep (130 registers): hide the reuse
#pragma unroll
        for (int t = 0; t < C; ++t) asm volatile("" : "+v"(xr[t]));
        if (!in_nan) {
            const double E = wave_exscan_add(X);
            // ---- pass 2 (straight line): pole-zero recurrence in the reference's operation order, in place
            const double c = c_row;
            double xp = (double)xprev, acc = E - c * (E - xp);
            float run = 0.0f;
            // the float32 prefix sum at every group end stays in registers, element 1 + group; element 0: nothing in front.  The carries
            // pick three of them at the plan's wave-uniform positions by indexed register moves
            typedef float fside __attribute__((ext_vector_type(NG + 1)));
            fside gend;
            gend[0] = zero;
#pragma unroll
            for (int t = 0; t < C; ++t) {
                if ((t & 7) == 0) __builtin_amdgcn_sched_barrier(0);
                const double x = t < KD ? xd[t] : (double)xr[t];
                // acc_k = acc_{k-1} + (x_k - c x_{k-1}); the float64 association differs from the reference's (acc + x) - xp*c by
                // <= 1 ulp of a double (the chunk carry already does), invisible after the float32 store; the chain is one add long
                acc += __builtin_fma(-c, xp, x);
                const float y = (float)acc;
                xr[t] = y;
                // other lanes read it with a lag; stored as pairs: 4-byte stores at the even pitch land two lanes on one bank
                if (t & 1) {
                    mine2[t >> 1] = f2{xr[t - 1], y};
                    RR_NO_MERGE();
                }
                xp = x;
                run += y;
                if ((t & 7) == 7) gend[(t >> 3) + 1] = run;
            }
            wave_sync();
            if constexpr (LATE) {
                fetch_next();
                fetched = true;
            }
            PHASE(2)
        RR_PRIO_AT(2)
            bool pz_nan = false;
            if (wave_any(!(fabsf(run) <= 3.4028234663852886e38f))) {
                bool n = false;
#pragma unroll
                for (int t = 0; t < C; ++t) n |= (xr[t] != xr[t]);
                pz_nan = wave_any(n);
            }
            if (pz_nan) {
                report(DSP_E_PZ_NAN, row);
            } else if (!A.all_nan && !(ABLATE(A) & 4) && pickoff_in_range(t_in, len)) {
                // ---- speculative carries
                const double Ep = wave_exscan_add((double)run);
                float g[S], y[S];
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    double Ak[3];
                    float pbase[3], pv[3][8];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        pbase[k] = gend[(pnpack[s] >> (12 + 5 * k)) & 31];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {  // (reads at most 6 past the chunk: inside the slot tail)
                            const f2 v = capp[k][s][u];
                            RR_NO_MERGE();
                            pv[k][2 * u] = v.x;
                            pv[k][2 * u + 1] = v.y;
                        }
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        // all eight running prefixes of the group, then the one the plan names: P[i] has the bits the sum of the first i
                        // samples had when the other 8 - i terms were added as +0.0f (the first addition to +0.0f makes every P[i], i >= 1,
                        // a sum that cannot be -0.0f, so a trailing + 0.0f changed nothing).  pn is wave-uniform: one indexed register move
                        float p[9];
                        p[0] = zero;
#pragma unroll
                        for (int u = 0; u < 8; ++u) p[u + 1] = p[u] + pv[k][u];
                        const f9 P = {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8]};
                        const float part = P[(pnpack[s] >> (4 * k)) & 15];
                        Ak[k] = wave_shift_up(Ep + (double)(pbase[k] + part), PL.shift[k][s]);
                    }
                    const double own = Ep + (s ? (double)gend[s * NGS] : 0.0);
                    double Gd;
                    if (KIND == TRAP_FILTER)
                        Gd = ((own - Ak[0]) - Ak[1]) + Ak[2];
                    else if (KIND == TRAP_NORM)
                        Gd = (((own - Ak[0]) - Ak[1]) + Ak[2]) / A.rr;
                    else
                        Gd = (own - Ak[0]) / A.rr - (Ak[1] - Ak[2]) / A.ll;
                    g[s] = (lane == 0 && s == 0) ? -0.0f : (float)Gd;
                    y[s] = g[s];
                }
                PHASE(3)
        RR_PRIO_AT(3)
                // ---- pass 3: replay; own samples from registers, the three lagged streams software-pipelined PD stages of GL = 4 samples ahead
                // Only the 4-point mode reads the replay's state at the group starts (its two 8-sample re-runs): that build writes them into
                // aux, which nothing else uses (the carries take pass 2's prefix sums from registers); the last row's re-runs read aux in
                // front of the wave_sync() that ends a row.  No build needs an ordering point here: the replay's lagged reads of other
                // lanes' pass-2 output are behind the wave_sync() that closes pass 2, and the pick-off samples it catches stay in registers.
                // the two samples every pick-off mode needs (floor and ceil of the time point) are caught on the fly: stage numbers
                const int i0 = (int)t_in;
                int capst[2], capoff[2], caplane[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int e = i0 + k;
                    const bool ok = e >= 0 && e < len;
                    caplane[k] = ok ? e / C : 0;
                    capoff[k] = ok ? e - caplane[k] * C : 0;
                    capst[k] = ok ? capoff[k] / BS : -1;  // capture block of the chunk; block (C-2)/BS (never reached) = the two-sample tail
                }
                // one test per BS samples (a not-taken branch still costs tens of cycles): bit q set = block q holds a wanted sample
                int capmask = (capst[0] >= 0 ? 1 << capst[0] : 0) | (capst[1] >= 0 ? 1 << capst[1] : 0);
                const bool ok1 = capst[1] >= 0;  // (sample i0 itself always exists here: 0 <= t_in <= len - 1)
                asm volatile("" : "+s"(capmask));  // one live scalar, not a recomputation at each test
                // ... and every lane keeps element capoff % BS of its own window of that block: a wave-uniform index, one indexed register move;
                // the tail's readlane at caplane[] then names the lane that owns the sample (no lane test, no trip through LDS)
                typedef float fbs __attribute__((ext_vector_type(BS)));
                // (readfirstlane: where the compiler had moved the index arithmetic to the vector unit -- the 2048-sample build -- it indexed
                // with sixteen compares and selects a pick instead)
                const int capidx[2] = {__builtin_amdgcn_readfirstlane(capoff[0] % BS), __builtin_amdgcn_readfirstlane(capoff[1] % BS)};
                float capv[2] = {0.0f, 0.0f};
                float ytail[2];  // the replay's output at the two samples of the tail
                // The lagged streams are read as aligned 8-byte pairs.  With the parity par[k] of lag k a compile-time constant, "element
                // t + par[k] of the pair sequence" names a register in this straight-line code: one copy of the replay per parity case,
                // chosen by one uniform switch per row (a wavefront runs the same copy for the whole launch).
                auto replay = [&](auto p0, auto p1, auto p2) __attribute__((always_inline)) {
                    constexpr int par[3] = {decltype(p0)::value, decltype(p1)::value, decltype(p2)::value};
                    constexpr int GL = 4, NL = CS / GL;  // samples per pipeline stage of the lagged streams
                    // stages the lagged loads run ahead of their use (lgkmcnt counts to 15: 6*S reads per stage).  8192 samples: one stage; its 130
                    // samples a lane leave no registers for a second stage of pairs in flight, the compiler parks values in AGPRs and copies
                    // them back inside the dependent chain (profiles/r05_headline_lds.md, "8192 samples: one stage ahead or two", has both measured)
                    constexpr int PD = S == 1 && NPF < 32 ? 2 : 1;
                    constexpr int NPS = CS / 2 + 2;      // pairs a sub-chain can need: CS / 2, one more for an odd lag, one more for the tail
                    f2 lp[3][S][NPS];
                    const f2* lagb2[3] = {reinterpret_cast<const f2*>(lagb[0]), reinterpret_cast<const f2*>(lagb[1]), reinterpret_cast<const f2*>(lagb[2])};
                    fbs ysb[S];
                    // stage st of sub-chain s consumes elements 4 st + par .. 4 st + 3 + par: an odd lag's stage ends in the first half of the
                    // pair after it, so its loads are the pairs [rr_pair_lo(st), rr_pair_lo(st + 1)) -- two per stage and stream either way, the
                    // first stage one more, stage NL (the tail, last sub-chain only) the one pair that is left
                    auto load_stage = [&](int st) __attribute__((always_inline)) {
#pragma unroll
                        for (int s = 0; s < S; ++s)
#pragma unroll
                            for (int jj = 0; jj < 3; ++jj)
#pragma unroll
                                for (int k = 0; k < 3; ++k) {
                                    const int np = (CS + (s == S - 1 ? 2 : 0) + par[k] + 1) / 2;  // pairs sub-chain s needs of stream k
                                    const int j = rr_pair_lo(st, par[k], np) + jj;
                                    if (j < rr_pair_lo(st + 1, par[k], np)) {
                                        lp[k][s][j] = lagb2[k][s * (CS / 2) + j];
                                        RR_NO_MERGE();
                                    }
                                }
                    };
                    auto lagged = [&](int k, int s, int t) __attribute__((always_inline)) { return lp[k][s][(t + par[k]) >> 1][(t + par[k]) & 1]; };
#pragma unroll
                    for (int st = 0; st < PD; ++st) load_stage(st);
#pragma unroll
                    for (int gl = 0; gl < NL; ++gl) {
                        __builtin_amdgcn_sched_barrier(0);
                        load_stage(gl + PD);  // (nothing past stage NL)
                        if (WIDE && (gl * GL) % 8 == 0) {  // (the re-runs' start states)
#pragma unroll
                            for (int s = 0; s < S; ++s) aux[s * NGS + (gl * GL) / 8] = y[s];
                        }
                        __builtin_amdgcn_sched_barrier(0);  // the reads just issued are younger than the stage consumed next: a counted wait
#pragma unroll
                        for (int u = 0; u < GL; ++u)
#pragma unroll
                            for (int s = 0; s < S; ++s) {
                                const int t = gl * GL + u;
                                y[s] = trap_step_r<float, KIND>(y[s], xr[s * CS + t], lagged(0, s, t), lagged(1, s, t), lagged(2, s, t), A.rr, A.ll, inv_rr, inv_ll);
                                ysb[s][t % BS] = y[s];
                            }
                        if (((gl + 1) * GL) % BS == 0) {
#pragma unroll
                            for (int s = 0; s < S; ++s) {
                                const int q = s * (CS / BS) + (gl * GL) / BS;
                                if (capmask & (1 << q)) {  // uniform, taken at most twice per waveform
#pragma unroll
                                    for (int k = 0; k < 2; ++k)
                                        if (capst[k] == q) capv[k] = ysb[s][capidx[k]];
                                }
                            }
                        }
                    }
                    if (WIDE) aux[S * NGS] = y[S - 1];  // state before the two-sample tail (it extends the last chain)
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        y[S - 1] = trap_step_r<float, KIND>(y[S - 1], xr[C - 2 + u], lagged(0, S - 1, CS + u), lagged(1, S - 1, CS + u), lagged(2, S - 1, CS + u),
                                                          A.rr, A.ll, inv_rr, inv_ll);
                        ytail[u] = y[S - 1];
                    }
                };
                {
                    typedef std::integral_constant<int, 0> E;  // even lag
                    typedef std::integral_constant<int, 1> O;  // odd lag
                    // trap_filter / trap_norm: the lags are rise, rise + flat, 2 rise + flat, so the third parity is the sum of the other two and
                    // four cases exist; asym_trap's fall time makes the third lag's parity free
                    if constexpr (KIND == TRAP_ASYM) {
                        switch (lagpar[0] | (lagpar[1] << 1) | (lagpar[2] << 2)) {
                            case 0: replay(E{}, E{}, E{}); break;
                            case 1: replay(O{}, E{}, E{}); break;
                            case 2: replay(E{}, O{}, E{}); break;
                            case 3: replay(O{}, O{}, E{}); break;
                            case 4: replay(E{}, E{}, O{}); break;
                            case 5: replay(O{}, E{}, O{}); break;
                            case 6: replay(E{}, O{}, O{}); break;
                            default: replay(O{}, O{}, O{}); break;
                        }
                    } else {
                        switch (lagpar[0] | (lagpar[1] << 1)) {
                            case 0: replay(E{}, E{}, E{}); break;
                            case 1: replay(O{}, E{}, O{}); break;
                            case 2: replay(E{}, O{}, O{}); break;
                            default: replay(O{}, O{}, E{}); break;
                        }
                    }
                }
                PHASE(4)
        RR_PRIO_AT(4)
                // ---- true carries: exact scan of the increments
                double D[S], Dbefore[S], Dtot = 0.0;
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    D[s] = (double)y[s] - (double)g[s];
                    Dbefore[s] = Dtot;
                    Dtot += D[s];
                }
                const double T0 = wave_exscan_add(Dtot);
                // ---- the two samples every mode needs, out of the capture buffer (or the tail's registers), with their lane's true carry
                float w4[4];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    float v = capv[k];  // (0.0f when the sample is in the tail or out of range: not used then)
                    v = capoff[k] >= C - 2 ? (capoff[k] == C - 2 ? ytail[0] : ytail[1]) : v;
                    double delta = T0 - (double)g[0];
#pragma unroll
                    for (int s = 1; s < S; ++s)
                        if (capoff[k] >= s * CS) delta = (T0 + Dbefore[s]) - (double)g[s];
                    w4[1 + k] = (k == 0 || ok1) ? readlane((float)((double)v + delta), caplane[k]) : 0.0f;
                }
                if constexpr (!WIDE) {
                    // ---- the two-point modes n f c l i (and an unknown mode's error), straight line: the expressions of pickoff_eval
                    // (dsp_wave.h), all evaluated, the mode and "t_in is a whole number" applied as selects on wave-uniform values.  (A time
                    // between two samples has both in range: t_in <= len - 1.)
                    const int mode = A.mode;
                    const double t0 = (double)t_in - (double)i0, t1 = 1.0 - t0;
                    const float lin = (float)(t1 * (double)w4[1] + t0 * (double)w4[2]);
                    const bool whole = (float)i0 == t_in, lo = t0 < 0.5;
                    const bool take1 = whole || mode == 'f' || (mode == 'n' && lo), take2 = mode == 'c' || (mode == 'n' && !lo);
                    result = take1 ? w4[1] : (take2 ? w4[2] : (mode == 'l' ? lin : quiet_nan<float>()));
                    const int fc = (take1 || take2 || mode == 'l') ? 0 : (mode == 'i' ? DSP_E_FTP_INT : DSP_E_FTP_MODE);
                    if (fc) report(fc, row);
                } else {
                    // ---- the 4-point mode h: its outer two samples by re-running the one 8-sample group that holds each from its saved start state
#pragma unroll
                    for (int k = 0; k < 4; k += 3) {
                        const int e = i0 - 1 + k;
                        const bool need = e >= 0 && e < len;
                        w4[k] = 0.0f;
                        __builtin_amdgcn_sched_barrier(0);
                        if (need) {  // uniform
                            const int l = e / C, off = e - l * C;
                            int ch = off / CS;
                            if (ch > S - 1) ch = S - 1;
                            const int loc = off - ch * CS;  // 0..CS+1 (CS, CS+1: the two-sample tail, chain S-1 only)
                            const int gi = loc >> 3, u0 = loc & 7;
                            float ys = aux[ch * NGS + gi], gsel = 0.0f;  // (chain S-1, group NGS) -> aux[S*NGS]
                            double dsel = 0.0;
#pragma unroll
                            for (int s = 0; s < S; ++s)
                                if (ch == s) {
                                    gsel = g[s];
                                    dsel = Dbefore[s];
                                }
                            const int base = ch * CS + gi * 8;
                            float yk = ys;
#pragma unroll
                            for (int u = 0; u < 8; ++u) {
                                const int tt = base + u;  // (beyond the chunk for the tail's group: reads stay in the slot tail, unused)
                                // (4-byte reads at a run-time position: no parity case needed, and the 4-point mode alone comes here.  At the even
                                // pitch they put two lanes on a bank, (2 lane + tt) mod 32: twice the array cycles, for 32 reads at most twice a row)
                                ys = trap_step_r<float, KIND>(ys, mine[tt], lagb[0][tt + lagpar[0]], lagb[1][tt + lagpar[1]], lagb[2][tt + lagpar[2]], A.rr, A.ll,
                                                              inv_rr, inv_ll);
                                if (u == u0) yk = ys;
                            }
                            const double delta = (T0 + dsel) - (double)gsel;
                            w4[k] = readlane((float)((double)yk + delta), l);
                        }
                    }
                    int fc = 0;
                    result = pickoff_eval(t_in, (int)'h', len, w4, fc);
                    if (fc) report(fc, row);
                }
            }
        }
        if (LATE && !fetched) fetch_next();  // a NaN row: it did not reach the prefetch behind pass 2
        pend_result = result;
        pend_row = row;
        // keeps the next row's staging stores (and, in the 4-point build, its replay's stores into aux) behind this row's lagged reads and
        // re-runs: all it orders since the pick-off samples stay in registers.  (dsp_wave.h: a fence for the compiler)
        wave_sync();
        PHASE(5)
        RR_PRIO_AT(5)
    }
    if (pend_row >= 0 && lane == 0) A.out[pend_row * A.out_stride] = pend_result;
    if (stamps && lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) atomicAdd(reinterpret_cast<unsigned long long*>(err + 4) + i, tsum[i]);
    }
}

// This file is two translation units (build.py compiles it twice; the kernels are templates in an unnamed namespace, each unit holds the
// instantiations it launches): unit 0, the file as it stands, has the classic kernel and the register-resident kernel of the two-point
// pick-off modes; unit 1 (dsp_energy_h.hip: DSP_ENERGY_UNIT 1 and this file included) has the register-resident kernel of the 4-point
// mode h -- the only code that holds the two 8-sample re-runs.  The pick-off mode is fixed for a chain's life; the host knows it at the launch.
#ifndef DSP_ENERGY_UNIT
#define DSP_ENERGY_UNIT 0
#endif

template <int KIND, int S, int IN, bool TAU = false>
int launch_rr_kind(const EnergyArgs& A, const EnergyPlan& PL, int npf, int64_t n_wf, int* err, int blocks, int threads, int lds_bytes,
                   hipStream_t st) {
    constexpr bool W = DSP_ENERGY_UNIT == 1;
    switch (npf) {
        case 4: hipLaunchKernelGGL((dsp_energy_rr_kernel<4, KIND, S, IN, TAU, W>), dim3(blocks), dim3(threads), lds_bytes, st, A, PL, n_wf, err); break;
        case 8: hipLaunchKernelGGL((dsp_energy_rr_kernel<8, KIND, S, IN, TAU, W>), dim3(blocks), dim3(threads), lds_bytes, st, A, PL, n_wf, err); break;
        case 16: hipLaunchKernelGGL((dsp_energy_rr_kernel<16, KIND, S, IN, TAU, W>), dim3(blocks), dim3(threads), lds_bytes, st, A, PL, n_wf, err); break;
        case 32:  // 8192 samples (production LEGEND rows): 130 samples per lane, one wavefront per SIMD (512-register budget, 38.9 KB of LDS)
            if (S != 1) return (int)hipErrorInvalidValue;
            hipLaunchKernelGGL((dsp_energy_rr_kernel<32, KIND, 1, IN, TAU, W>), dim3(blocks), dim3(threads), lds_bytes, st, A, PL, n_wf, err);
            break;
        default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

// S = sub-chains of the trapezoid replay (1: default, 2: measured slower, kept for A/B, float32 rows only); wf_dtype = DSP_F32 / DSP_I16 / DSP_U16 rows
int launch_rr(const EnergyArgs* A, const EnergyPlan* PL, int trap_opcode, int npf, int S, int wf_dtype, int64_t n_wf, int* err, int blocks,
              int threads, int lds_bytes, hipStream_t stream) {
#define GO_(KIND)                                                                                                          \
    if (A->tau && wf_dtype == DSP_I16) return launch_rr_kind<KIND, 1, 1, true>(*A, *PL, npf, n_wf, err, blocks, threads, lds_bytes, stream); \
    if (A->tau && wf_dtype == DSP_U16) return launch_rr_kind<KIND, 1, 2, true>(*A, *PL, npf, n_wf, err, blocks, threads, lds_bytes, stream); \
    if (A->tau) return launch_rr_kind<KIND, 1, 0, true>(*A, *PL, npf, n_wf, err, blocks, threads, lds_bytes, stream);       \
    if (wf_dtype == DSP_I16) return launch_rr_kind<KIND, 1, 1>(*A, *PL, npf, n_wf, err, blocks, threads, lds_bytes, stream); \
    if (wf_dtype == DSP_U16) return launch_rr_kind<KIND, 1, 2>(*A, *PL, npf, n_wf, err, blocks, threads, lds_bytes, stream); \
    return S == 2 ? launch_rr_kind<KIND, 2, 0>(*A, *PL, npf, n_wf, err, blocks, threads, lds_bytes, stream)                \
                  : launch_rr_kind<KIND, 1, 0>(*A, *PL, npf, n_wf, err, blocks, threads, lds_bytes, stream);
    if (trap_opcode == DSP_OP_TRAP_FILTER) { GO_(TRAP_FILTER) }
    if (trap_opcode == DSP_OP_TRAP_NORM) { GO_(TRAP_NORM) }
    GO_(TRAP_ASYM)
#undef GO_
}

#if DSP_ENERGY_UNIT == 0
template <int KIND>
int launch_kind(const EnergyArgs& A, int npf, int64_t n_wf, int* err, int blocks, int threads, int lds_bytes, hipStream_t s) {
    switch (npf) {
        case 4: hipLaunchKernelGGL((dsp_energy_kernel<4, KIND>), dim3(blocks), dim3(threads), lds_bytes, s, A, n_wf, err); break;
        case 8: hipLaunchKernelGGL((dsp_energy_kernel<8, KIND>), dim3(blocks), dim3(threads), lds_bytes, s, A, n_wf, err); break;
        case 16: hipLaunchKernelGGL((dsp_energy_kernel<16, KIND>), dim3(blocks), dim3(threads), lds_bytes, s, A, n_wf, err); break;
        case 32: hipLaunchKernelGGL((dsp_energy_kernel<32, KIND>), dim3(blocks), dim3(threads), lds_bytes, s, A, n_wf, err); break;
        default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

}  // namespace

// npf = number of 16-byte loads per lane that cover one waveform: 4, 8, 16 or 32 (C = 4*npf)
extern "C" int dsp_internal_launch_energy(const EnergyArgs* A, int trap_opcode, int npf, int64_t n_wf, int* err, int blocks,
                                          int threads, int lds_bytes, hipStream_t stream) {
    if (trap_opcode == DSP_OP_TRAP_FILTER) return launch_kind<TRAP_FILTER>(*A, npf, n_wf, err, blocks, threads, lds_bytes, stream);
    if (trap_opcode == DSP_OP_TRAP_NORM) return launch_kind<TRAP_NORM>(*A, npf, n_wf, err, blocks, threads, lds_bytes, stream);
    return launch_kind<TRAP_ASYM>(*A, npf, n_wf, err, blocks, threads, lds_bytes, stream);
}

extern "C" int dsp_internal_set_energy_lds(int trap_opcode, int npf, int lds_bytes) {
#define SET_(NPF, KIND)                                                                                                   \
    if (npf == NPF && kind == KIND)                                                                                        \
        return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(&dsp_energy_kernel<NPF, KIND>),                      \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    const int kind = trap_opcode == DSP_OP_TRAP_FILTER ? TRAP_FILTER : (trap_opcode == DSP_OP_TRAP_NORM ? TRAP_NORM : TRAP_ASYM);
    SET_(4, TRAP_FILTER) SET_(8, TRAP_FILTER) SET_(16, TRAP_FILTER) SET_(32, TRAP_FILTER)
    SET_(4, TRAP_NORM) SET_(8, TRAP_NORM) SET_(16, TRAP_NORM) SET_(32, TRAP_NORM)
    SET_(4, TRAP_ASYM) SET_(8, TRAP_ASYM) SET_(16, TRAP_ASYM) SET_(32, TRAP_ASYM)
#undef SET_
    return (int)hipErrorInvalidValue;
}

// register-resident kernel, plan[S - 1]: the build for the chain's pick-off mode class (mode h: unit 1)
extern "C" int dsp_internal_launch_energy_rr(const EnergyArgs* A, const EnergyPlan* PL, int trap_opcode, int npf, int S, int wf_dtype,
                                             int64_t n_wf, int* err, int blocks, int threads, int lds_bytes, hipStream_t stream) {
    return (A->mode == 'h' ? dsp_internal_launch_energy_rr_h : launch_rr)(A, PL, trap_opcode, npf, S, wf_dtype, n_wf, err, blocks, threads, lds_bytes, stream);
}
#else
}  // namespace

extern "C" int dsp_internal_launch_energy_rr_h(const EnergyArgs* A, const EnergyPlan* PL, int trap_opcode, int npf, int S, int wf_dtype,
                                               int64_t n_wf, int* err, int blocks, int threads, int lds_bytes, hipStream_t stream) {
    return launch_rr(A, PL, trap_opcode, npf, S, wf_dtype, n_wf, err, blocks, threads, lds_bytes, stream);
}
#endif
