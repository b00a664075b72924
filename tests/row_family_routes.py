"""What the CPU oracle alone gives on the waveform families of tests/row_families.py, route by route: the per-row inputs every route
needs beside the rows (baselines, thresholds, pick-off times, window starts), chosen so that every output is finite in at least half of a
batch's rows, and the oracle's outputs for them.  tests/test_row_families_cpu.py checks these on their own (return codes, finite
fractions); tests/test_gpu_row_families.py compares the device with them.  No device code here.

Every function returns (inputs, want): two dicts of arrays with one entry per row."""
import numpy as np

import golden_util
import oracle
import row_families as rf

F = np.float32


def _ok(res):
    """(outputs..., rc) of an oracle call -> the outputs, once the reference would not have raised"""
    *out, rc = res
    assert rc == 0, oracle.E_NAMES.get(rc, rc)
    return out[0] if len(out) == 1 else out


def blsub(b):
    """the rows with their pedestal subtracted, float32 (the oracle's bl_subtract)"""
    return _ok(oracle.bl_subtract(b.rows.astype(F), b.pedestal))


def _mixed_thresholds(b, row_max, sample_values, seed, level=None):
    """Per-row thresholds: every second row a fraction 0.1 .. 0.9 of that row's oracle maximum (so that every pulse family has crossings), the
    others cycle through constants -- a negative one, a small and a large one -- and a value that equals a sample of the row exactly.
    level: where the filtered row rests ahead of the pulse when that is not zero; the constants are counted from there."""
    rng = np.random.default_rng([seed, len(b)])
    n = len(b)
    thr = (rng.uniform(0.1, 0.9, n) * row_max.astype(np.float64)).astype(F)
    for r in range(1, n, 2):
        k = (r // 2) % 4
        thr[r] = sample_values[r] if k == 3 else F((0.0 if level is None else level[r]) + (-2.0, 20.0, 200.0)[k])
    return thr


# ---- R1: bl_subtract -> pole_zero -> trap_filter -> fixed_time_pickoff (the energy chain)
def r1(b, rise, flat, mode="l", tau=None):
    """tau: None (the recipes' constant) or "per_event" (each row's own decay constant as a column)"""
    n = b.rows.shape[1]
    tp = np.where(np.isfinite(b.onset), b.onset + rise + 0.8 * flat, n // 2 + 0.8 * flat).astype(F)  # (`late` rows: beyond the row)
    w = b.rows.astype(F)
    inp = {"baseline": b.pedestal, "t_pick": tp}
    if tau is None:
        want = _ok(oracle.chain_energy(w, b.pedestal, tp, rf.TAU, rise, flat, mode))
        trap = _ok(oracle.chain_pz_trap(w - b.pedestal[:, None], rf.TAU, rise, flat))
    else:
        taus = np.full(len(b), rf.TAU, F)
        taus[b.of("tau_short")] = F(0.5 * rf.TAU)
        taus[b.of("tau_long")] = F(2.0 * rf.TAU)
        inp["tau"] = taus
        xs = blsub(b)
        trap = np.empty_like(xs)
        want = np.empty(len(b), F)
        for r in range(len(b)):
            trap[r] = _ok(oracle.trap_filter(_ok(oracle.pole_zero(xs[r:r + 1], float(taus[r]))), rise, flat))[0]
            want[r] = _ok(oracle.fixed_time_pickoff(trap[r], tp[r:r + 1], mode))[0]
    return inp, {"trapEftp": want, "_peak": np.max(np.abs(trap), axis=1)}


# ---- R2: [bl_subtract ->] pole_zero | double_pole_zero -> short trapezoid -> min_max, time_point_thresh, Haar DWT (lane per waveform)
DPZ = ("double_pole_zero", 1716.28, 62.5, 0.02)
PZ = ("pole_zero", 1716.28)
ATRAP = ("asym_trap_filter", 8, 4, 125)
# (the rise a power of two, where the kernel multiplies by 1 / rise, and not, where it divides; normalised and not)
R2_FORMS = [(8192, "interleaved", "C5", ATRAP), (2048, "interleaved", "bl", ATRAP), (2048, "sorted", "bl", ATRAP),
            (2048, "interleaved", "bl", ("trap_norm", 24, 9)), (2048, "sorted", "bl", ("asym_trap_filter", 10, 6, 100)),
            (2048, "interleaved", "bl", ("trap_filter", 40, 13))]


def r2(b, pz, trap, with_bl, dwt_level=5):
    """with_bl: the recipe subtracts the baseline column itself.  Otherwise (recipes.C5) signed rows go in as they are and rows on a pedestal of
    10 000 with it taken off beforehand, as float32: the filters' start-up on such a pedestal is the row's maximum and no walk finds a crossing."""
    rows = b.rows if with_bl or b.rows.dtype == np.int16 else blsub(b)
    w = blsub(b) if with_bl else rows.astype(F)
    w1 = _ok(oracle.pole_zero(w, pz[1]) if pz[0] == "pole_zero" else oracle.double_pole_zero(w, *pz[1:]))
    w2 = _ok(getattr(oracle, trap[0])(w1, *trap[1:]))
    tmin, tmax, amin, amax = _ok(oracle.min_max(w2))
    at = np.clip(tmax.astype(np.int64) - 3, 0, None)  # a sample on the flank below the maximum: the walk meets it exactly
    # (without a baseline subtraction the pole-zero stage turns the pedestal into a ramp and the trapezoid into an offset of some hundreds)
    thr = _mixed_thresholds(b, amax, w2[np.arange(len(b)), at], 2, level=np.median(w2[:, 200:600], axis=1))
    tp0 = _ok(oracle.time_point_thresh(w2, thr, tmax, 0))
    dwt = _ok(oracle.dwt_haar(w1, dwt_level, "a", w.shape[1] >> dwt_level))
    return {"waveform": rows, "thr": thr, "baseline": b.pedestal}, {"tp_min": tmin, "tp_max": tmax, "wf_min": amin, "wf_max": amax, "tp_0": tp0, "dwt": dwt}


# ---- R3: pole-zero rows with the raw rows' min_max beside them; min_max / amax / walks straight off raw rows
def r3_pz(b):
    w = b.rows.astype(F)
    tmin, tmax, amin, amax = _ok(oracle.min_max(w))
    pz = _ok(oracle.pole_zero(blsub(b), 1716.28))
    return {"baseline": b.pedestal}, {"t_lo": tmin, "t_hi": tmax, "v_lo": amin, "v_hi": amax, "wf_pz": pz}


def r3_reduce(b):
    """walk0: backward from t_max, walk1: forward from t_min, both with the per-row threshold; on `saturated` rows the threshold is the
    plateau's value itself"""
    w = b.rows.astype(F)
    tmin, tmax, amin, amax = _ok(oracle.min_max(w))
    rng = np.random.default_rng([3, len(b)])
    thr = (amin + rng.uniform(0.1, 0.9, len(b)) * (amax.astype(np.float64) - amin)).astype(F)  # (a fraction of the row's span: raw rows sit on a pedestal)
    third = np.arange(len(b)) % 3 == 1
    thr[third] = w[np.arange(len(b)), np.clip(tmax.astype(np.int64) - 3, 0, None)][third]  # a sample's own value: on integer rows a tie
    thr[b.of("saturated")] = F(rf.sample_range(b.rows.dtype)[1])
    want = {"t_min": tmin, "t_max": tmax, "a_min": amin, "a_max": amax, "amax": np.max(w, axis=1),
            "walk0": _ok(oracle.time_point_thresh(w, thr, tmax, 0)), "walk1": _ok(oracle.time_point_thresh(w, thr, tmin, 1))}
    return {"thr": thr}, want


# ---- R4: FIR filters
def fir_bar_scales(want, taps, x):
    """the two terms of the FIR bar per row, each already divided into the 1e-6 / 2e-7 they carry: (peak of the filtered row, sum|k| max|x|)"""
    return np.max(np.abs(want), axis=1).astype(np.float64), float(np.abs(taps.astype(np.float64)).sum()) * np.max(np.abs(x), axis=1).astype(np.float64)


def r4_c3(b):
    """recipes.C3: cusp and zero-area cusp (5792 taps, the reference generators' own: golden fixtures) over the first 6092 samples, 'valid'"""
    x = blsub(b)
    want = {}
    for nm in ("cusp", "zac"):
        k = golden_util.recipe_kernel(nm)
        conv = _ok(oracle.convolve_wf(x, k, "v", 301, in_len=6092))
        want[f"{nm}Emax"] = np.max(conv, axis=1)
        want[f"_peak:{nm}"], want[f"_dot:{nm}"] = fir_bar_scales(conv, k, x[:, :6092])
    return {"baseline": b.pedestal}, want


def r4_stored(b, taps):
    """a stored 'same' convolution of the baseline-subtracted rows with `taps` (the product's t0_filter taps of that geometry)"""
    x = blsub(b)
    conv = _ok(oracle.convolve_wf(x, taps, "s", x.shape[1]))
    peak, dot = fir_bar_scales(conv, taps, x)
    return {"baseline": b.pedestal}, {"wf_f": conv, "_peak": peak, "_dot": dot}


def r4_runs(b):
    """the Ge recipes' t0 filter (8 + 125 taps, golden) in 'same' mode over baseline-subtracted float32 rows, with min_max of the filtered
    row, a walk back from its maximum and one forward from sample 100"""
    x = blsub(b)
    taps = golden_util.recipe_kernel("t0")
    conv = _ok(oracle.convolve_wf(x, taps, "s", x.shape[1]))
    amax = np.max(conv, axis=1)
    at = np.clip(np.argmax(conv, axis=1) - 3, 0, None)
    thr = _mixed_thresholds(b, amax, conv[np.arange(len(b)), at], 4)
    peak, dot = fir_bar_scales(conv, taps, x)
    return {"x": x, "taps": taps, "thr": thr}, {"filtered": conv, "_peak": peak, "_dot": dot}


# ---- R5: trapezoids straight on integer rows
def r5_cases(rise, flat):
    """(name, processor call, oracle of the filtered row, readers) as tests/test_gpu_nonfinite_chains._trap_cases, at an energy trapezoid's size"""
    fall = rise // 2
    return [
        ("trap_filter", f"trap_filter(waveform, {rise}, {flat}, wf_t)", lambda w: _ok(oracle.trap_filter(w, rise, flat)), "min_max+tpt"),
        ("trap_norm", f"trap_norm(waveform, {rise}, {flat}, wf_t)", lambda w: _ok(oracle.trap_norm(w, rise, flat)), "amax"),
        ("asym_trap", f"asym_trap_filter(waveform, {rise}, {flat}, {fall}, wf_t)", lambda w: _ok(oracle.asym_trap_filter(w, rise, flat, fall)), "tpt_fwd"),
        ("trap_pickoff", f"trap_filter(waveform, {rise}, {flat}, wf_t)", lambda w: _ok(oracle.trap_filter(w, rise, flat)), "pickoff"),
    ]


def r5(b, case, rise, flat):
    """A threshold equal to a sample of the row is a tie only where the device's row is the oracle's bit for bit: `trap_filter` does not
    divide, so on integer rows every running value is an integer, exact in float32 in any order of summation while the row's peak stays
    below 2^24 (want["_exact"]).  Every other row gets, in that slot of the cycle, the value half way between two neighbouring samples of
    the flank: a crossing that a deviation inside the bar does not move."""
    name, _call, filt, red = case
    n = b.rows.shape[1]
    f = filt(b.rows.astype(F))
    amax = np.max(f, axis=1)
    r = np.arange(len(b))
    at = np.clip(np.argmax(f, axis=1) - 3, 0, None)
    exact = (np.max(np.abs(f), axis=1) < 2 ** 24) if name in ("trap_filter", "trap_pickoff") else np.zeros(len(b), bool)
    between = (0.5 * (f[r, at].astype(np.float64) + f[r, at + 1])).astype(F)
    thr = _mixed_thresholds(b, amax, np.where(exact, f[r, at], between), 5)
    tp = (np.where(np.isfinite(b.onset), b.onset + rise + 0.8 * flat, n // 2 + 0.8 * flat)).astype(F)
    return {"thr": thr, "t_pick": tp}, {"wf_t": f, "_exact": exact}


# ---- R6: the current branch and the fits, a waveform per lane
def oracle_onset(x):
    """where the oracle's short asymmetric trapezoid of a baseline-subtracted row last rises through half its maximum (NaN: nowhere)"""
    at = _ok(oracle.asym_trap_filter(x, 8, 4, 125))
    _tmin, tmax, _amin, amax = _ok(oracle.min_max(at))
    return _ok(oracle.time_point_thresh(at, (F(0.5) * amax).astype(F), tmax, 0))


def r6_current(b, n_win=301):
    x = blsub(b)
    n = x.shape[1]
    onset = oracle_onset(x)
    # (`early`: the window starts before the row, `late`: it runs off the row's end -> NaN; no onset: mid-row)
    start = np.where(np.isfinite(onset), onset - 40, n // 2).astype(F)
    w = _ok(oracle.windower(x, start, n_win))
    a = _ok(oracle.moving_window_multi(_ok(oracle.upsampler(_ok(oracle.avg_current(w, 1)), 16, 4784)), 48, 3, 0))
    t_lo, t_hi, a_lo, a_hi = _ok(oracle.min_max(a))
    return {"wf": x, "t_start": start}, {"t_lo": t_lo, "t_hi": t_hi, "a_lo": a_lo, "a_hi": a_hi}


R6_FITS = [(0, 0, 700), (1, 1500, 548), (0, 100, 50)]  # (stage: 0 baseline-subtracted / 1 pole-zero rows, first sample, count) at 2048 samples


def r6_fits(b, tau=1716.25):
    y = blsub(b)
    z = _ok(oracle.pole_zero(y, tau))
    res = []
    for stage, first, count in R6_FITS:
        src = z if stage else y
        res.append(np.stack(_ok(oracle.linear_slope_fit(np.ascontiguousarray(src[:, first:first + count])))))
    return {"baseline": b.pedestal}, {"fits": np.stack(res)}


# ---- R7: the whole Ge recipe
def r7_t0_ns(n_rows):
    """a time of the first sample per row, on the 16 ns grid (as the whole-recipe tests draw it)"""
    return (np.random.default_rng([7, n_rows]).integers(2900, 3100, n_rows) * 16).astype(F)


def r7_scales(b, par):
    """what the whole recipe's float outputs are measured against, from the oracle's own intermediate rows: the peak of every filtered row, and
    sum|k| max|x| of the three FIRs; par: recipes.ICPC_PARAMS / ICPC_REF_PARAMS"""
    x = blsub(b)
    pz = _ok(oracle.pole_zero(x, F(par["tau_samples"])))
    peak = lambda w: np.max(np.abs(w.astype(np.float64)), axis=1)  # noqa: E731
    sc = {"pz": peak(pz), "trap": peak(_ok(oracle.trap_norm(pz, 625, 188))), "etrap": peak(_ok(oracle.trap_norm(pz, *par["etrap"]))),
          "trap2": peak(_ok(oracle.trap_norm(pz, 250, 6)))}
    sc["dot:t0"] = float(np.abs(golden_util.recipe_kernel("t0").astype(np.float64)).sum()) * peak(pz)
    for nm in ("cusp", "zac"):
        k = golden_util.recipe_kernel(nm)
        sc[nm] = peak(_ok(oracle.convolve_wf(x, k, "v", 301, in_len=8192 - 2100)))
        sc[f"dot:{nm}"] = float(np.abs(k.astype(np.float64)).sum()) * peak(x[:, :8192 - 2100])
    return sc


def r7_current_peak(b, par, tp0):
    """peak of the oracle's averaged current row (what A_max is picked off), on the oracle's own window start tp0 (a sample index per row)"""
    pz = _ok(oracle.pole_zero(blsub(b), F(par["tau_samples"])))
    up = oracle.upsampler(oracle.avg_current(oracle.windower(pz, tp0, 301)[0], 1)[0], 16, 4784)[0]
    av = oracle.moving_window_multi(up, 48, 3, 0)[0]
    return np.max(np.where(np.isfinite(av), np.abs(av.astype(np.float64)), 0.0), axis=1)


# ---- caps of the issue: every output finite in at least half of the rows, and in every `control` row
def finite_rows(v):
    v = np.asarray(v)
    return np.isfinite(v) if v.ndim == 1 else np.isfinite(v).all(axis=tuple(range(1, v.ndim)))


def check_caps(b, want, what):
    for k, v in want.items():
        if k.startswith("_"):
            continue
        if k == "fits":
            v = np.moveaxis(v, -1, 0)  # (fits, 4, rows) -> rows first
        ok = finite_rows(v)
        assert ok.sum() * 2 >= len(b), f"{what} {k}: finite in {int(ok.sum())} of {len(b)} rows"
        assert ok[b.of("control")].all(), f"{what} {k}: a NaN in a control row"
