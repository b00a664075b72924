"""Programs, batch layout and oracle-side expectations of tests/test_gpu_vm_row_loop.py (the device) and tests/test_vm_row_loop_cases_cpu.py
(do the cases say something? -- the planner and the oracle alone).  Nothing here needs a GPU; everything is seeded.

What is aimed at: the interpreter's wavefronts are persistent.  A wavefront clears its LDS region once, at kernel start, and then runs
row base + wave, base + wave + total_waves, ... on that region (dsp_vm.hip, "zero the whole region once").  From its second row on, the
guards below the slots, the pads and partial last chunks, the slots that take over another slot's region (DSP_OP_INTERNAL_ZERO), the
NaN flags, the scalar registers and the op scratch area all start as the previous row left them.  So every program here is run on a
batch in which each wavefront gets three or four rows: a probe, a poison row, the same probe again, another probe (``layout``).

Every program is a recipe for build_processing_chain, kept whole on the interpreter by the switches of ``WHOLE`` (``switches``)."""
import contextlib
import functools
import os

import numpy as np

import oracle
from dspeed_amd import _lib

M = "dspeed.processors"
F = np.float32
TAU = 1716.28

#: no specialised kernel, no stage ahead of the program, the fits inside it, nothing cut off its head or tail, no reductions off the rows
WHOLE = {"DSPEED_HIP_NO_FUSED": "1", "DSPEED_HIP_NO_STAGES": "1", "DSPEED_HIP_FIT_IN_CHAIN": "1", "DSPEED_HIP_NO_SCALAR_TAIL": "1",
         "DSPEED_HIP_NO_SCALAR_HEAD": "1", "DSPEED_HIP_NO_WALKS_BEHIND": "1", "DSPEED_HIP_NO_ROW_REDUCTIONS": "1"}
TEAM_SWITCHES = ("DSPEED_HIP_NO_TEAMS", "DSPEED_HIP_TEAM_MAX", "DSPEED_HIP_TEAM_WPB")

L = _lib
#: the opcodes of the interpreter's switch (dsp_vm.hip, dsp_vm_kernel: `switch (op.opcode)` of the TEAM == 1 build) that a recipe's program
#: can hold.  Its three other labels are made by the planner, never by a recipe: DSP_OP_INTERNAL_ZERO (a slot that shares LDS: programs 1
#: to 3, see the CPU test), DSP_OP_INTERNAL_STORES (two scalar stores in a row: every program) and DSP_OP_INTERNAL_NOP (a folded threshold)
INTERPRETER_OPCODES = sorted([
    L.OP_LOAD, L.OP_STORE, L.OP_STORE_SCALAR, L.OP_BL_SUBTRACT, L.OP_MIN_MAX_NORM, L.OP_POLE_ZERO, L.OP_DOUBLE_POLE_ZERO, L.OP_TRAP_FILTER,
    L.OP_TRAP_NORM, L.OP_ASYM_TRAP, L.OP_PICKOFF, L.OP_TRAP_PICKOFF, L.OP_TRAP_REDUCE, L.OP_UPSAMPLER, L.OP_LINEAR_SLOPE_FIT,
    L.OP_MOVING_WINDOW_MULTI, L.OP_TIME_POINT_THRESH, L.OP_INTERP_TIME_POINT_THRESH, L.OP_MIN_MAX, L.OP_AMAX, L.OP_MEAN_BELOW, L.OP_WINDOWER,
    L.OP_AVG_CURRENT, L.OP_TRAP_WINDOW_PICKOFF, L.OP_DWT_HAAR, L.OP_COPY, L.OP_CONVOLVE, L.OP_CONVOLVE_AMAX, L.OP_SCALAR_AFFINE,
    L.OP_SCALAR_DIV, L.OP_ELEMENTWISE, L.OP_SCALAR_FUNC, L.OP_SCALAR_CONVERT])

N_PROBES = 32
#: probes whose thresholds lie above every sample: their walks find no crossing
NO_CROSSING = (28, 29, 30, 31)
POISON = ("all-nan", "nan-last", "inf-ends", "huge-alternating", "all-zero", "denormal", "nan-scalar", "time-outside", "threshold-unreached")
#: the kinds an integer row cannot hold; such a row gets the extremes it can hold in their place (``poison_waveform``)
FLOAT_ONLY = ("all-nan", "nan-last", "inf-ends", "huge-alternating", "denormal")
ROUND3_SHIFT = 11  # round 3 of slot s holds probe (s + 11) % 32: never the probe of rounds 0 and 2


@contextlib.contextmanager
def switches(extra=None):
    """the environment that keeps a recipe whole on the interpreter, + ``extra`` (the team switches); put back on exit.  The planner reads it
    when the chain is created, the compiler when the recipe is translated: build, create and run inside"""
    env = dict(WHOLE, **(extra or {}))
    names = set(env) | set(TEAM_SWITCHES)
    old = {k: os.environ.get(k) for k in names}
    for k in TEAM_SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _ok(res):
    *out, rc = res
    assert rc == 0, rc
    return out[0] if len(out) == 1 else out


def layout(S):
    """row -> index into the table of N_PROBES + len(POISON) distinct rows, for a launch that takes S rows per round: 3 S + S // 2 rows, row r
    on slot r % S in round r // S.  Round 0: probe slot % 32; round 1: poison kind slot % 9 (9 and 32 share no factor: every probe meets
    every kind); round 2: round 0 again; round 3, half of the slots: another probe"""
    r = np.arange(3 * S + S // 2)
    slot, rnd = r % S, r // S
    probe = np.where(rnd == 3, (slot + ROUND3_SHIFT) % N_PROBES, slot % N_PROBES)
    return np.where(rnd == 1, N_PROBES + slot % len(POISON), probe)


def rows_per_round(geometry, team):
    """S of a launch whose rows are at least as many as its row slots (chain.geometry(n) of a large n)"""
    waves = geometry["blocks"] * geometry["waves_per_block"]
    assert waves % team == 0, (geometry, team)
    return waves // team


# ------------------------------------------------------------------------------------------------------------------------------------
# rows
# ------------------------------------------------------------------------------------------------------------------------------------
def pulses(length, seed, n=N_PROBES, bl=(-3000, 3000), amp=(500, 15000), rise=(1, 11)):
    """n distinct pulses (float64): a baseline, a rise of rise[0] to rise[1] - 1 samples that starts at 0.3 .. 0.6 of the row, an exponential tail, noise.
    Returns (rows, baselines, amplitudes, start samples)"""
    rng = np.random.default_rng(seed)
    i = np.arange(length, dtype=np.float64)[None, :]
    B = rng.uniform(*bl, (n, 1))
    A = rng.uniform(*amp, (n, 1))
    t0 = np.floor(rng.uniform(0.3, 0.6, (n, 1)) * length)
    rise = rng.integers(*rise, (n, 1)).astype(np.float64)
    d = i - t0
    x = B + A * np.exp(-np.clip(d, 0, None) / TAU) * np.clip((d + 1) / rise, 0, 1) + 5.0 * rng.standard_normal((n, length))
    return x, B[:, 0], A[:, 0], t0[:, 0]


def _as_rows(x, dtype):
    return np.rint(x).astype(dtype) if np.dtype(dtype).kind in "iu" else x.astype(dtype)


def poison_waveform(kind, probe, dtype, inf_at_0=True):
    """the samples of a poison row made from ``probe`` (a row of the batch's type); None: the kind leaves the samples alone.
    ``inf_at_0`` False: a program whose rows go through pole_zero keeps only the -inf in the last sample -- an infinite sample anywhere before
    it makes that filter's state inf - inf, which is the reference's DSPFatal ("NaN in output", pole_zero.py:76-77), not a result"""
    dtype = np.dtype(dtype)
    w = probe.copy()
    n = len(w)
    if dtype.kind in "iu":
        hi, lo = np.iinfo(dtype).max, np.iinfo(dtype).min
        if kind == "all-nan":
            w[:] = lo
        elif kind == "nan-last":
            w[:] = hi
        elif kind == "inf-ends":
            w[0], w[-1] = hi, lo
        elif kind == "huge-alternating":
            w[:] = np.where(np.arange(n) % 2 == 0, hi, -hi if dtype.kind == "i" else 0)
        elif kind == "denormal":
            w[:] = np.where(np.arange(n) % 2 == 0, 1, -1 if dtype.kind == "i" else 0)
        elif kind == "all-zero":
            w[:] = 0
        else:
            return None
        return w
    if kind == "all-nan":
        w[:] = np.nan
    elif kind == "nan-last":
        w[-1] = np.nan
    elif kind == "inf-ends":
        w[-1] = -np.inf
        if inf_at_0:
            w[0] = np.inf
    elif kind == "huge-alternating":
        w[:] = np.where(np.arange(n) % 2 == 0, 3e38, -3e38)
    elif kind == "all-zero":
        w[:] = 0
    elif kind == "denormal":
        # the samples within 40 counts of the pedestal -- everything ahead of the pulse -- as denormals of the row's type around zero, the
        # pulse itself on a zero pedestal: a row of mostly denormal samples whose outputs still have a peak to measure against
        d = probe.astype(np.float64) - np.median(probe[:n // 4].astype(np.float64))  # (no pulse starts before 0.3 of the row)
        with np.errstate(under="ignore"):
            w[:] = np.where(np.abs(d) < 40, d * (1e-42 if dtype == F else 1e-310), d).astype(dtype)
        assert np.count_nonzero((w != 0) & (np.abs(w) < np.finfo(dtype).tiny)) > n // 4
    else:
        return None
    return w


def with_poison(cols, wf_name, scalar_poison, inf_at_0=True):
    """the table of N_PROBES probe rows ``cols`` + one row per poison kind, each made from probe 0.  ``scalar_poison``: kind -> {column: value}
    for the kinds that poison a per-event value; 'all-zero' and 'denormal' take the 'all-zero' entry (a zero baseline beside the samples)"""
    out = {k: np.concatenate([v, np.repeat(v[:1], len(POISON), axis=0)]) for k, v in cols.items()}
    for j, kind in enumerate(POISON):
        r = N_PROBES + j
        w = poison_waveform(kind, cols[wf_name][0], cols[wf_name].dtype, inf_at_0)
        if w is not None:
            out[wf_name][r] = w
        for name, value in scalar_poison.get("all-zero" if kind == "denormal" else kind, {}).items():
            out[name][r] = value
    for v in out.values():
        v.setflags(write=False)
    return out


class Case:
    """One program at one length: ``recipe``; ``table()``: the N_PROBES + len(POISON) distinct rows, name -> column; ``want(table)``: name ->
    (oracle column, bar), bar 'exact' | ('peak', oracle rows whose largest finite magnitude per row scales the tolerance, 'filter' | 'dpz');
    ``env``: switches beside WHOLE; ``team``: wavefronts per row the planner must choose; ``float_rows``: the rows can hold NaN"""

    def __init__(self, name, program, recipe, table, want, ft=F, env=None, team=1, float_rows=True, inputs=None):
        self.name, self.program, self.recipe, self._table, self._want = name, program, recipe, table, want
        self.ft, self.env, self.team, self.float_rows = np.dtype(ft), dict(env or {}), team, float_rows
        self.inputs = inputs  # name -> wrapper of the column as the recipe reads it (a WaveformInput with its grid)

    @functools.lru_cache(maxsize=None)
    def table(self):
        return self._table()

    @functools.lru_cache(maxsize=None)
    def want(self):
        with np.errstate(all="ignore"):
            return self._want(self.table())

    def linked(self, cols):
        """``cols`` as build_processing_chain / ProcessingChain.link take them"""
        return {k: (self.inputs[k](v) if self.inputs and k in self.inputs else v) for k, v in cols.items()}

    def build(self, rows=4):
        """(chain, output table) of the recipe translated for the first ``rows`` distinct rows (call inside ``switches(self.env)``)"""
        from dspeed_amd.processing_chain import build_processing_chain

        chain, _, out = build_processing_chain(self.recipe, self.linked({k: v[:rows] for k, v in self.table().items()}))
        assert not chain._stages and not chain._aux and chain._tail is None and chain._walks is None  # (one program, one launch)
        return chain, out


def _proc(fn, *args, module=M):
    return {"function": fn, "module": module, "args": list(args)}


# ------------------------------------------------------------------------------------------------------------------------------------
# program 1 (and 6): bl_subtract -> pole_zero -> the four filters, each stored; every kind of read-off
# ------------------------------------------------------------------------------------------------------------------------------------
P1_TRAP, P1_NORM, P1_ASYM, P1_DPZ = (20, 8), (16, 4), (8, 4, 40), (TAU, 62.5, 0.02)
P1_MM = ("t_lo", "t_hi", "a_lo", "a_hi")
P1_WAVEFORMS = ("wf_dpz", "wf_tf", "wf_tn", "wf_at")  # (wf_bl and wf_pz are not: their regions are free for the filters' outputs)
P1_MODES = "nlhs"
P1_HEAD = (8, 72)  # a window of wf_pz that is copied into a slot of its own: free again before the filters' outputs are placed


def filters_recipe(stored=P1_WAVEFORMS):
    procs = {
        "wf_bl": f"{M}.bl_subtract(waveform, baseline, wf_bl)",
        "wf_pz": _proc("pole_zero", "wf_bl", str(TAU), "wf_pz"),
        "wf_dpz": _proc("double_pole_zero", "wf_pz", *map(str, P1_DPZ), "wf_dpz"),
        "wf_tf": _proc("trap_filter", "wf_pz", *map(str, P1_TRAP), "wf_tf"),
        "wf_tn": _proc("trap_norm", "wf_pz", *map(str, P1_NORM), "wf_tn"),
        "wf_at": _proc("asym_trap_filter", "wf_pz", *map(str, P1_ASYM), "wf_at"),
        "tn_max": _proc("amax", "wf_tn", 1, "tn_max", module="numpy"),
        "pz_head": _proc("amax", f"wf_pz[{P1_HEAD[0]}:{P1_HEAD[1]}]", 1, "pz_head", module="numpy"),
        ", ".join(P1_MM): _proc("min_max", "wf_at", *P1_MM),
        "tp_b": f"{M}.time_point_thresh(wf_at, thr, t_hi, 0, tp_b)",
        "tp_f": f"{M}.time_point_thresh(wf_bl, thr_f, t_start, 1, tp_f)",
        "tp_i": f"{M}.interpolated_time_point_thresh(wf_bl, thr_f, t_start, 1, 'l', tp_i)",
        "e_tp": f"{M}.trap_pickoff(wf_bl, {P1_TRAP[0]}, {P1_TRAP[1]}, t_int, e_tp)"}
    for m in P1_MODES:
        procs[f"e_{m}"] = _proc("fixed_time_pickoff", "wf_bl", "t_pick", f"'{m}'", f"e_{m}")
    scalars = ["tn_max", "pz_head", *P1_MM, "tp_b", "tp_f", "tp_i", "e_tp"] + [f"e_{m}" for m in P1_MODES]
    return {"outputs": scalars + list(stored), "processors": procs}


def filters_table(length, dtype, seed):
    ft = np.float64 if np.dtype(dtype) == np.float64 else F
    x, B, A, t0 = pulses(length, seed)
    rng = np.random.default_rng(seed + 1)
    thr, thr_f = rng.uniform(0.1, 0.6, N_PROBES) * A, rng.uniform(0.2, 0.8, N_PROBES) * A
    thr[list(NO_CROSSING)] = thr_f[list(NO_CROSSING)] = 1e6
    t_pick = t0 + rng.uniform(5, 40, N_PROBES)
    t_pick[3] = np.floor(t_pick[3])  # (a whole sample: every mode returns it)
    cols = {"waveform": _as_rows(x, dtype), "baseline": B.astype(ft), "thr": thr.astype(ft), "thr_f": thr_f.astype(ft),
            "t_start": (t0 - rng.integers(10, 30, N_PROBES)).astype(ft), "t_pick": t_pick.astype(ft),
            "t_int": np.floor(t0 + rng.uniform(0, 30, N_PROBES)).astype(ft)}
    assert cols["t_start"].min() >= 0 and t_pick.max() <= length - 3 and cols["t_int"].min() + 1 >= 2 * P1_TRAP[0] + P1_TRAP[1]
    return with_poison(cols, "waveform", {
        "all-zero": {"baseline": 0.0}, "nan-scalar": {"baseline": np.nan}, "time-outside": {"t_pick": length + 6.0, "t_int": length + 6.0},
        "threshold-unreached": {"thr": 3e38, "thr_f": 3e38}}, inf_at_0=False)


def filters_want(tb, stored=P1_WAVEFORMS):
    ft = tb["baseline"].dtype
    o = oracle
    w = {"wf_bl": _ok(o.bl_subtract(tb["waveform"].astype(ft), tb["baseline"]))}
    w["wf_pz"] = _ok(o.pole_zero(w["wf_bl"], TAU))
    w["wf_dpz"] = _ok(o.double_pole_zero(w["wf_pz"], *P1_DPZ))
    w["wf_tf"] = _ok(o.trap_filter(w["wf_pz"], *P1_TRAP))
    w["wf_tn"] = _ok(o.trap_norm(w["wf_pz"], *P1_NORM))
    w["wf_at"] = _ok(o.asym_trap_filter(w["wf_pz"], *P1_ASYM))
    exact_or = lambda rows: "exact" if ft == F else ("peak", rows, "filter")  # noqa: E731  (float64 sums run in another order on the device)
    want = {k: (w[k], "exact" if k == "wf_bl" else ("peak", w[k], "dpz" if k == "wf_dpz" else "filter")) for k in stored}
    want["tn_max"] = (np.max(w["wf_tn"], axis=1), ("peak", w["wf_tn"], "filter"))  # (numpy.amax: NaN wins)
    head = w["wf_pz"][:, P1_HEAD[0]:P1_HEAD[1]]
    want["pz_head"] = (np.where(np.isnan(w["wf_pz"]).any(axis=1), np.nan, np.max(head, axis=1)).astype(ft), ("peak", w["wf_pz"], "filter"))
    mm = _ok(o.min_max(w["wf_at"]))
    for k, v in zip(P1_MM, mm):
        want[k] = (v, "exact" if k.startswith("t_") else ("peak", w["wf_at"], "filter"))
    want["tp_b"] = (_ok(o.time_point_thresh(w["wf_at"], tb["thr"], mm[1], 0)), "exact")
    want["tp_f"] = (_ok(o.time_point_thresh(w["wf_bl"], tb["thr_f"], tb["t_start"], 1)), "exact")
    want["tp_i"] = (_ok(o.interpolated_time_point_thresh(w["wf_bl"], tb["thr_f"], tb["t_start"], 1, "l")), "exact")
    want["e_tp"] = (_ok(o.trap_pickoff(w["wf_bl"], *P1_TRAP, tb["t_int"])), exact_or(w["wf_bl"]))
    for m in P1_MODES:
        want[f"e_{m}"] = (_ok(o.fixed_time_pickoff(w["wf_bl"], tb["t_pick"], m)), exact_or(w["wf_bl"]))
    return want


def _filters_case(program, length, dtype, stored=P1_WAVEFORMS):
    dtype = np.dtype(dtype)
    return Case(f"p{program}-filters-{length}-{dtype.name}", program, filters_recipe(stored),
                functools.partial(filters_table, length, dtype, 1000 * program + length), functools.partial(filters_want, stored=stored),
                ft=np.float64 if dtype == np.float64 else F, float_rows=dtype.kind == "f")


# ------------------------------------------------------------------------------------------------------------------------------------
# program 2: the current branch -- slots of 1024, 150, 149, 1100 and 64 x 40 samples: each its own chunk and pitch, and they take over each
# other's regions
# ------------------------------------------------------------------------------------------------------------------------------------
P2 = dict(n_win=150, ac=1, up=8, n_up=1100, ma=40)
P2_LEN = 1024
P2_MM = ("t_lo", "t_hi", "a_lo", "a_hi")


def current_recipe():
    n_win, ac = P2["n_win"], P2["ac"]
    return {"outputs": [*P2_MM, "tp_c", "w_first"], "processors": {
        "wf_le": f"{M}.windower(wf, t_start, wf_le({n_win}, 'f'))",
        "curr": f"{M}.avg_current(wf_le, {ac}, curr({n_win - ac}, 'f'))",
        "curr_up": f"{M}.upsampler(curr, {P2['up']}, curr_up({P2['n_up']}, 'f'))",
        "curr_av": f"{M}.moving_window_multi(curr_up, {P2['ma']}, 3, 0, curr_av)",
        ", ".join(P2_MM): _proc("min_max", "curr_av", *P2_MM),
        "tp_c": f"{M}.time_point_thresh(curr_av, thr, t_hi, 0, tp_c)",
        "w_first": _proc("fixed_time_pickoff", "wf_le", "3", "'n'", "w_first")}}  # (ahead of the pulse: the window starts 20 samples or more before it)


def current_table(seed=2000):
    x, _B, A, t0 = pulses(P2_LEN, seed, bl=(-50, 50))
    rng = np.random.default_rng(seed + 1)
    rise = 5.0  # (the pulses rise within 1 to 10 samples: the current's peak is about A / rise, the threshold a fraction of the least of them)
    thr = rng.uniform(0.02, 0.08, N_PROBES) * A / rise
    thr[list(NO_CROSSING)] = 1e6
    start = t0 - rng.integers(20, 60, N_PROBES)
    start[5] += 0.37  # (a fractional start truncates)
    cols = {"wf": x.astype(F), "t_start": start.astype(F), "thr": thr.astype(F)}
    # (one sample past the last window that fits: the window's last sample is outside the row, NaN in a slot that holds real samples)
    # (the row with the infinities is windowed from sample 0: the +inf is in the window)
    return with_poison(cols, "wf", {"inf-ends": {"t_start": 0.0}, "nan-scalar": {"t_start": np.nan}, "time-outside": {"t_start": P2_LEN - P2["n_win"] + 1.0},
                                    "threshold-unreached": {"thr": 3e38}})


def current_want(tb):
    o = oracle
    w = _ok(o.windower(tb["wf"], tb["t_start"], P2["n_win"]))
    c = _ok(o.avg_current(w, P2["ac"]))
    u = _ok(o.upsampler(c, P2["up"], P2["n_up"]))
    a = _ok(o.moving_window_multi(u, P2["ma"], 3, 0))
    mm = _ok(o.min_max(a))
    want = {k: (v, "exact" if k.startswith("t_") else ("peak", a, "filter")) for k, v in zip(P2_MM, mm)}
    want["tp_c"] = (_ok(o.time_point_thresh(a, tb["thr"], mm[1], 0)), "exact")
    want["w_first"] = (_ok(o.fixed_time_pickoff(w, F(3), "n")), "exact")
    return want


# ------------------------------------------------------------------------------------------------------------------------------------
# program 3: the build with the FIR op -- short kernels (20, 32 and 48 taps: below every specialised kernel's admission) on a slice of the
# row in the three modes, the Haar transform, a fit and a mean inside the program
# ------------------------------------------------------------------------------------------------------------------------------------
P3_LEN, P3_SLICE, P3_FIT, P3_DWT = 1000, (100, 700), (0, 300), (3, 125)
P3_TAPS = {"k_s": 20, "k_f": (8, 24), "k_v": 48}
P3_FITS = ("f_mean", "f_std", "f_slope", "f_icpt")


def moving_slope_taps(n):
    """the least-squares slope of n samples as FIR weights, (n j - S1) / (n S2 - S1^2) for j = n .. 1, numerator and denominator rounded to
    float32 before the division (the reference's generator, processors/kernels.py:69-100, restated)"""
    s1, s2 = n * (n + 1) / 2, n * (n + 1) * (2 * n + 1) / 6
    return (n * np.arange(n, 0, -1, dtype=np.float64) - s1).astype(F) / F(n * s2 - s1 * s1)


def t0_taps(rise, fall):
    """a ramp 2 (r - i) / (r (r + 1)) of `rise` weights, then the plateau -1 / fall (processors/kernels.py:12-61, restated)"""
    return np.concatenate([2.0 * np.arange(rise, 0, -1) / (rise * (rise + 1)), np.full(fall, -1.0 / fall)]).astype(F)


def fir_taps():
    return {"k_s": moving_slope_taps(P3_TAPS["k_s"]), "k_f": t0_taps(*P3_TAPS["k_f"]), "k_v": moving_slope_taps(P3_TAPS["k_v"])}


def fir_recipe():
    lo, hi = P3_SLICE
    n, (r, f) = hi - lo, P3_TAPS["k_f"]
    src = f"wf_bl[{lo}:{hi}]"
    return {"outputs": ["wf_s", "wf_f", "c_max", "e_s", "dwt", *P3_FITS, "mb"], "processors": {
        "wf_bl": f"{M}.bl_subtract(waveform, baseline, wf_bl)",
        "k_s": _proc("moving_slope", f"k_s({P3_TAPS['k_s']}, 'f')"),
        "k_f": _proc("t0_filter", str(r), str(f), f"k_f({r + f}, 'f')"),
        "k_v": _proc("moving_slope", f"k_v({P3_TAPS['k_v']}, 'f')"),
        "wf_s": _proc("convolve_wf", src, "k_s", "'s'", f"wf_s({n}, 'f')"),
        "wf_f": _proc("convolve_wf", src, "k_f", "'f'", f"wf_f({n + r + f - 1}, 'f')"),
        "wf_v": _proc("convolve_wf", src, "k_v", "'v'", f"wf_v({n - P3_TAPS['k_v'] + 1}, 'f')"),
        "c_max": _proc("amax", "wf_v", 1, "c_max", module="numpy"),
        "e_s": _proc("fixed_time_pickoff", "wf_s", "t_pick", "'l'", "e_s"),
        "dwt": _proc("discrete_wavelet_transform", "wf_bl", P3_DWT[0], "'h'", "'a'", f"dwt({P3_DWT[1]}, 'f')"),
        ", ".join(P3_FITS): _proc("linear_slope_fit", f"wf_bl[{P3_FIT[0]}:{P3_FIT[1]}]", *P3_FITS),
        "mb": f"{M}.mean_below_threshold(wf_bl, thr_m, mb)"}}


def fir_table(seed=3000):
    x, B, A, t0 = pulses(P3_LEN, seed)
    rng = np.random.default_rng(seed + 1)
    thr_m = rng.uniform(0.2, 0.8, N_PROBES) * A
    thr_m[list(NO_CROSSING)] = -1e6  # (nothing lies below: the mean of no sample)
    cols = {"waveform": x.astype(F), "baseline": B.astype(F), "thr_m": thr_m.astype(F),
            "t_pick": (t0 - P3_SLICE[0] + rng.uniform(-20, 60, N_PROBES)).astype(F)}
    assert cols["t_pick"].min() >= 0 and cols["t_pick"].max() <= P3_SLICE[1] - P3_SLICE[0] - 2
    return with_poison(cols, "waveform", {"all-zero": {"baseline": 0.0}, "nan-scalar": {"baseline": np.nan},
                                          "time-outside": {"t_pick": P3_LEN + 6.0}, "threshold-unreached": {"thr_m": -3e38}})


def fir_want(tb):
    o, taps = oracle, fir_taps()
    lo, hi = P3_SLICE
    n = hi - lo
    bl = _ok(o.bl_subtract(tb["waveform"], tb["baseline"]))
    src = np.ascontiguousarray(bl[:, lo:hi])
    nan_row = np.isnan(bl).any(axis=1)  # (a slice of a waveform with a NaN anywhere in it is NaN: the reference's processors see the whole variable)
    src[nan_row] = np.nan
    s = _ok(o.convolve_wf(src, taps["k_s"], "s", n))
    f = _ok(o.convolve_wf(src, taps["k_f"], "f", n + len(taps["k_f"]) - 1))
    v = _ok(o.convolve_wf(src, taps["k_v"], "v", n - len(taps["k_v"]) + 1))
    want = {"wf_s": (s, ("peak", s, "filter")), "wf_f": (f, ("peak", f, "filter")), "c_max": (np.max(v, axis=1), ("peak", v, "filter")),
            "e_s": (_ok(o.fixed_time_pickoff(s, tb["t_pick"], "l")), ("peak", s, "filter")),
            "dwt": (_ok(o.dwt_haar(bl, P3_DWT[0], "a", P3_DWT[1])), "exact"), "mb": (_ok(o.mean_below_threshold(bl, tb["thr_m"])), "exact")}
    win = np.ascontiguousarray(bl[:, P3_FIT[0]:P3_FIT[1]])
    win[nan_row] = np.nan
    mean, std, slope, icpt = _ok(o.linear_slope_fit(win))
    scale = np.max(np.abs(np.where(np.isfinite(win), win, 0)), axis=1)
    # (the bars of test_gpu_processors.py::test_linear_slope_fit_golden: mean and deviation run the oracle's sequence of operations; slope and
    # intercept come from float64 sums taken in another order)
    want.update(f_mean=(mean, "exact"), f_std=(std, "exact"), f_slope=(slope, ("close", 1e-6, 1e-6 * scale / win.shape[1])),
                f_icpt=(icpt, ("close", 1e-6, 1e-6 * scale)))
    return want


# ------------------------------------------------------------------------------------------------------------------------------------
# program 4: expressions between waveform variables and between registers; registers that only a walk assigns, which may find nothing
# ------------------------------------------------------------------------------------------------------------------------------------
P4_LEN, P4_PERIOD, P4_T0 = 1000, 16.0, 48000.0
P4_MM = ("t_a", "t_b", "lo", "hi")


def _wf_input(values):
    from dspeed_amd.processing_chain import WaveformInput

    return WaveformInput(values, P4_PERIOD, P4_T0)


def expr_recipe():
    return {"outputs": ["prod", "clean", "norm", "win", *P4_MM, "span", "ratio", "cent", "tp", "e_late", "e_pick", "neg"], "processors": {
        "a": "waveform - baseline",
        "prod": "a * other",
        "q": "a / other",
        "clean": "where(isnan(q), 0, q)",
        ", ".join(P4_MM): _proc("min_max", "a", *P4_MM),
        "norm": _proc("min_max_norm", "a", "lo", "hi", "norm"),
        "win": "a[100:200] - a[300:400]",
        "span": "hi - lo",
        "ratio": "lo / hi",
        "cent": "round(ratio * 100)",
        "tp": f"{M}.time_point_thresh(a, thr, t_b, 0, tp)",
        "e_late": _proc("fixed_time_pickoff", "a", "tp + 80*ns", "'n'", "e_late"),
        "e_pick": _proc("fixed_time_pickoff", "a", "t_pick", "'l'", "e_pick"),
        "neg": "-span if isnan(tp) else span"}}


def expr_table(seed=4000):
    x, B, A, _t0 = pulses(P4_LEN, seed)
    y, _B, _A, _t = pulses(P4_LEN, seed + 7, bl=(200, 900), amp=(100, 500))
    rng = np.random.default_rng(seed + 1)
    thr = rng.uniform(0.1, 0.6, N_PROBES) * A
    thr[list(NO_CROSSING)] = 1e6
    cols = {"waveform": x.astype(F), "other": y.astype(F), "baseline": B.astype(F), "thr": thr.astype(F),
            "t_pick": rng.uniform(10, P4_LEN - 10, N_PROBES).astype(F)}
    return with_poison(cols, "waveform", {"all-zero": {"baseline": 0.0}, "nan-scalar": {"baseline": np.nan}, "time-outside": {"t_pick": P4_LEN + 6.0},
                                          "threshold-unreached": {"thr": 3e38}})


def expr_want(tb):
    o = oracle
    # (numpy.subtract, not bl_subtract: a NaN sample stays one NaN sample; the processors that read `a` make the row NaN)
    a = np.where(np.isnan(tb["baseline"])[:, None], np.nan, tb["waveform"] - tb["baseline"][:, None]).astype(F)
    y = tb["other"]
    q = a / y
    want = {"prod": (a * y, "exact"), "clean": (np.where(np.isnan(q), F(0), q), "exact"), "win": (a[:, 100:200] - a[:, 300:400], "exact")}
    mm = _ok(o.min_max(a))
    want.update({k: (v, "exact") for k, v in zip(P4_MM, mm)})
    _ta, t_b, lo, hi = mm
    want["norm"] = (_ok(o.min_max_norm(a, lo, hi)), "exact")
    want["span"], want["ratio"] = (hi - lo, "exact"), (lo / hi, "exact")
    want["cent"] = (np.rint(lo / hi * F(100)), "exact")
    tp = _ok(o.time_point_thresh(a, tb["thr"], t_b, 0))
    want["tp"] = (tp, "exact")
    want["e_late"] = (_ok(o.fixed_time_pickoff(a, tp + F(5), "n")), "exact")
    want["e_pick"] = (_ok(o.fixed_time_pickoff(a, tb["t_pick"], "l")), "exact")
    want["neg"] = (np.where(np.isnan(tp), -(hi - lo), hi - lo), "exact")
    return want


# ------------------------------------------------------------------------------------------------------------------------------------
# program 5: a load and then only readers, in the shape of the Ge recipe's tail -- groups of ops that share no register, dealt out to a
# team of wavefronts on one LDS image
# ------------------------------------------------------------------------------------------------------------------------------------
P5_LEN = 8192
P5_E, P5_Q, P5_A = (500, 125), (250, 6), (8, 4, 125)
P5_MM = ("t_lo", "t_hi", "a_lo", "a_hi")
P5_TEAMS = {"team3": ({}, 3), "team2": ({"DSPEED_HIP_TEAM_MAX": "2"}, 2), "team3-wpb4": ({"DSPEED_HIP_TEAM_WPB": "4"}, 3),
            "no-teams": ({"DSPEED_HIP_NO_TEAMS": "1"}, 1)}


def team_recipe():
    return {"outputs": ["e_max", "e_ftp", "q_ftp", "q_drift", "dt_eff", *P5_MM, "tp_0", "tp_100", "tp_90", "tp_50", "w_max", "e_h", "e_early"], "processors": {
        "wf_e": _proc("trap_norm", "wf_pz", *map(str, P5_E), "wf_e"),
        "e_max": _proc("amax", "wf_e", 1, "e_max", module="numpy"),
        "e_ftp": _proc("fixed_time_pickoff", "wf_e", "t_pick", "'l'", "e_ftp"),
        "wf_q": _proc("trap_norm", "wf_pz", *map(str, P5_Q), "wf_q"),
        "q_ftp": _proc("fixed_time_pickoff", "wf_q", "t_pick", "'l'", "q_ftp"),
        "q_drift": "q_ftp * 16",
        "dt_eff": "q_drift / e_max",
        "wf_a": _proc("asym_trap_filter", "wf_pz", *map(str, P5_A), "wf_a"),
        ", ".join(P5_MM): _proc("min_max", "wf_a", *P5_MM),
        "tp_0": f"{M}.time_point_thresh(wf_a, thr, t_hi, 0, tp_0)",
        "w_max": _proc("amax", "wf_pz", 1, "w_max", module="numpy"),
        "tp_100": f"{M}.time_point_thresh(wf_pz, 0.98*w_max, t_first, 1, tp_100)",
        "tp_90": f"{M}.time_point_thresh(wf_pz, w_max*0.9, tp_100, 0, tp_90)",
        "tp_50": f"{M}.time_point_thresh(wf_pz, w_max*0.5, tp_90, 0, tp_50)",
        "e_h": _proc("fixed_time_pickoff", "wf_pz", "t_pick", "'h'", "e_h"),
        "e_early": _proc("fixed_time_pickoff", "wf_pz", "t_first", "'n'", "e_early")}}


def team_table(seed=5000):
    x, _B, A, t0 = pulses(P5_LEN, seed, bl=(-20, 20), rise=(12, 40))  # (a rise the ladder of walks can stand on)
    rng = np.random.default_rng(seed + 1)
    thr = rng.uniform(0.1, 0.6, N_PROBES) * A
    thr[list(NO_CROSSING)] = 1e6
    cols = {"wf_pz": x.astype(F), "thr": thr.astype(F), "t_pick": (t0 + P5_E[0] + 0.8 * P5_E[1] + rng.uniform(0, 1, N_PROBES)).astype(F),
            "t_first": (t0 - rng.integers(100, 300, N_PROBES)).astype(F)}
    return with_poison(cols, "wf_pz", {"nan-scalar": {"thr": np.nan}, "time-outside": {"t_pick": P5_LEN + 6.0}, "threshold-unreached": {"thr": 3e38}})


def team_want(tb):
    o, w = oracle, tb["wf_pz"]
    e, q, a = _ok(o.trap_norm(w, *P5_E)), _ok(o.trap_norm(w, *P5_Q)), _ok(o.asym_trap_filter(w, *P5_A))
    e_max, w_max = np.max(e, axis=1), np.max(w, axis=1)
    q_ftp = _ok(o.fixed_time_pickoff(q, tb["t_pick"], "l"))
    want = {"e_max": (e_max, ("peak", e, "filter")), "e_ftp": (_ok(o.fixed_time_pickoff(e, tb["t_pick"], "l")), ("peak", e, "filter")),
            "q_ftp": (q_ftp, ("peak", q, "filter")), "q_drift": (q_ftp * F(16), ("peak", q * F(16), "filter")),
            "w_max": (w_max, "exact"), "e_h": (_ok(o.fixed_time_pickoff(w, tb["t_pick"], "h")), "exact"),
            "e_early": (_ok(o.fixed_time_pickoff(w, tb["t_first"], "n")), "exact")}
    mm = _ok(o.min_max(a))
    want.update({k: (v, "exact" if k.startswith("t_") else ("peak", a, "filter")) for k, v in zip(P5_MM, mm)})
    want["tp_0"] = (_ok(o.time_point_thresh(a, tb["thr"], mm[1], 0)), "exact")
    tp_100 = _ok(o.time_point_thresh(w, F(0.98) * w_max, tb["t_first"], 1))
    tp_90 = _ok(o.time_point_thresh(w, w_max * F(0.9), tp_100, 0))
    want.update(tp_100=(tp_100, "exact"), tp_90=(tp_90, "exact"), tp_50=(_ok(o.time_point_thresh(w, w_max * F(0.5), tp_90, 0)), "exact"))
    # dt_eff = q_drift / e_max: both within 1e-6 of their trapezoid's peak; the quotient is compared at the same bar, scaled by the quotient of
    # the peaks (e_max IS its trapezoid's peak)
    want["dt_eff"] = (q_ftp * F(16) / e_max, ("peak", (q * F(16)) / np.where(e_max == 0, 1, e_max)[:, None], "filter"))
    return want


@functools.lru_cache(maxsize=None)
def cases():
    """every program x length (x team configuration) the GPU module runs"""
    out = [_filters_case(1, 200, F), _filters_case(1, 1000, F), _filters_case(1, 1024, F), _filters_case(1, 8192, np.int16, stored=("wf_tf",)),
           Case(f"p2-current-{P2_LEN}", 2, current_recipe(), current_table, current_want),
           Case(f"p3-fir-{P3_LEN}", 3, fir_recipe(), fir_table, fir_want),
           Case(f"p4-expressions-{P4_LEN}", 4, expr_recipe(), expr_table, expr_want, inputs={"waveform": _wf_input, "other": _wf_input})]
    out += [Case(f"p5-{k}-{P5_LEN}", 5, team_recipe(), team_table, team_want, env=env, team=team) for k, (env, team) in P5_TEAMS.items()]
    out += [_filters_case(6, 1000, np.float64), _filters_case(6, 1024, np.float64)]
    return out
