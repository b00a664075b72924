"""Case tables, recipes, row generators and oracle pipelines of the three lane-per-waveform kernels (dsp_current.hip, dsp_rows.hip,
dsp_fit.hip), shared by test_lane_kernel_cases_cpu.py (do the cases say something? -- on the oracle alone) and
test_gpu_lane_kernel_variants.py (the device against the oracle, bit for bit).  Nothing here needs a GPU.  Every generator takes a seed:
the same rows in every process."""
import numpy as np

import oracle

M = "dspeed.processors"
N_ROWS = 70  # rows of a case unless it says otherwise (one full wavefront of waveforms and a partial one)


def scaled(x, factor):
    """float32 rows times ``factor``, rounded once (overflow to infinity and underflow to denormals included)"""
    with np.errstate(over="ignore", under="ignore"):
        return (np.asarray(x, dtype=np.float64) * factor).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------------------
# current branch: windower -> avg_current -> upsampler -> moving_window_multi(3, alternating) -> min_max
# ------------------------------------------------------------------------------------------------------------------------------------
CURRENT_NAMES = ("t_lo", "t_hi", "a_lo", "a_hi")
CURRENT_DEFAULT = dict(n_win=301, ac=1, up=16, n_up=4784, ma=48)
#: the admission limit ((n_up - 1 + up/2) >> log2 up) < n_c met with equality: the kernel reads the last increment D[n_c - 1], and one
#: element further lies another array (the checkpoint P0[0]); q = ma / 16
CURRENT_TIGHT = [dict(n_win=98, ac=1, up=2, n_up=192, ma=32),    # SH = 1; reads D[96], n_c = 97
                 dict(n_win=161, ac=1, up=1, n_up=160, ma=64),   # up 1, q = 4
                 dict(n_win=88, ac=3, up=4, n_up=336, ma=80),    # up 4, q = 5
                 dict(n_win=199, ac=2, up=8, n_up=1568, ma=96)]  # up 8, q = 6
CURRENT_SMALL = [dict(n_win=4, ac=1, up=16, n_up=32, ma=16),     # the smallest shape admitted: two blocks, q = 1
                 dict(n_win=10, ac=1, up=16, n_up=128, ma=112)]  # nb - q = 1: every block but one is head and tail at once
CURRENT_SCALES = (1e-42, 1e30, 3e34)


def current_id(p):
    return "win{n_win}-ac{ac}-up{up}-n{n_up}-ma{ma}".format(**p)


def current_refused(p):
    """the neighbour of a tight shape that the kernel must not take: a window one sample shorter"""
    return dict(p, n_win=p["n_win"] - 1)


def current_recipe(p, outputs=CURRENT_NAMES, start="t_start", src="wf"):
    n_win, ac = p["n_win"], p["ac"]
    return {"outputs": list(outputs), "processors": {
        "wf_le": f"{M}.windower({src}, {start}, wf_le({n_win}, 'f'))",
        "curr": f"{M}.avg_current(wf_le, {ac}, curr({n_win - ac}, 'f'))",
        "curr_up": f"{M}.upsampler(curr, {p['up']}, curr_up({p['n_up']}, 'f'))",
        "curr_av": f"{M}.moving_window_multi(curr_up, {p['ma']}, 3, 0, curr_av)",
        "t_lo, t_hi, a_lo, a_hi": f"{M}.min_max(curr_av, t_lo, t_hi, a_lo, a_hi)"}}


def current_oracle(wf, start, p):
    """{name: column} of the five processors run one after the other; every call must succeed"""
    w, rc = oracle.windower(wf, start, p["n_win"])
    assert rc == 0, ("windower", rc)
    c, rc = oracle.avg_current(w, p["ac"])
    assert rc == 0, ("avg_current", rc)
    u, rc = oracle.upsampler(c, p["up"], p["n_up"])
    assert rc == 0, ("upsampler", rc)
    a, rc = oracle.moving_window_multi(u, p["ma"], 3, 0)
    assert rc == 0, ("moving_window_multi", rc)
    *mm, rc = oracle.min_max(a)
    assert rc == 0, ("min_max", rc)
    return dict(zip(CURRENT_NAMES, mm))


def current_rows(seed, n=N_ROWS, length=1024):
    """charge-like float32 rows (the generator of test_gpu_current_kernel) and the sample each rise starts at"""
    rng = np.random.default_rng(seed)
    i = np.arange(length, dtype=np.float64)[None, :]
    t0 = np.floor(rng.uniform(0.3, 0.6, (n, 1)) * length)
    rise = rng.uniform(3, 40, (n, 1))
    x = rng.uniform(500, 15000, (n, 1)) * (1 - np.exp(-np.clip(i - t0, 0, None) / rise)) * np.exp(-np.clip(i - t0, 0, None) / 30000.0)
    x += 5 * rng.standard_normal((n, length))
    return x.astype(np.float32), t0[:, 0]


#: rows whose window start is special, and whether the window they name exists
CURRENT_SPECIAL_STARTS = {5: True, 6: True, 7: False, 8: True, 9: False, 10: False, 11: False}


def current_starts(seed, t0, length, n_win, special=True):
    """a window start per row, 20 to 60 samples ahead of the rise; ``special``: the starts of CURRENT_SPECIAL_STARTS in rows 5 .. 11"""
    rng = np.random.default_rng(seed)
    start = (t0 - rng.integers(20, 60, len(t0))).astype(np.float32)
    if special:
        start[5] += 0.37               # a fractional start truncates
        start[6] = -0.5                # int(-0.5) == 0: a window from sample 0
        start[7] = -1.0                # one sample before the waveform: NaN
        start[8] = length - n_win      # the last window that fits
        start[9] = length - n_win + 1  # one past: NaN
        start[10] = np.nan
        start[11] = 1e9
    return start


# ------------------------------------------------------------------------------------------------------------------------------------
# rows kernel: [bl_subtract ->] [pole_zero | double_pole_zero ->] short trapezoid -> min_max / time_point_thresh, Haar DWT
# ------------------------------------------------------------------------------------------------------------------------------------
PZ1 = ("pole_zero", 1716.28)
DPZ = ("double_pole_zero", 1716.28, 62.5, 0.02)
T0_TRAP = ("asym_trap_filter", 8, 4, 125)
MM_NAMES = ("tp_min", "tp_max", "wf_min", "wf_max")


def synth_rows(seed, n=N_ROWS, length=1024, bl=(-3000, 3000), amp=(500, 15000), dtype=np.int16):
    """step-like rows with an exponential tail (the generator of test_gpu_rows_kernel) and their baselines"""
    rng = np.random.default_rng(seed)
    i = np.arange(length, dtype=np.float64)[None, :]
    B = rng.uniform(*bl, (n, 1))
    A = rng.uniform(*amp, (n, 1))
    t0 = np.floor(rng.uniform(0.45, 0.55, (n, 1)) * length)
    x = B + A * np.exp(-(i - t0) / 1716.28) * (i >= t0) + 5.0 * rng.standard_normal((n, length))
    if np.dtype(dtype).kind in "iu":
        x = np.rint(x + (4000 if np.dtype(dtype).kind == "u" else 0))
    return x.astype(dtype), B[:, 0].astype(np.float32)


def thresholds(seed, n=N_ROWS, lo=5.0, hi=40.0):
    return np.random.default_rng(seed).uniform(lo, hi, n).astype(np.float32)


def rows_recipe(pz, trap, bl=None, tpt=None, dwt=None, mm=True):
    """pz: None | PZ1 | DPZ-like;  trap: (function, ints...);  bl: None | name of a column | a number;  tpt: None | (threshold, start, walk)
    as the recipe spells them;  dwt: None | (level, part, n_out);  mm: store the four values of min_max"""
    procs, src = {}, "waveform"
    if bl is not None:
        procs["wf_bl"] = f"{M}.bl_subtract(waveform, {bl}, wf_bl)"
        src = "wf_bl"
    if pz is not None:
        procs["wf_pz"] = {"function": pz[0], "module": M, "args": [src, *[str(v) for v in pz[1:]], "wf_pz"]}
        src = "wf_pz"
    procs["wf_tr"] = {"function": trap[0], "module": M, "args": [src, *[str(v) for v in trap[1:]], "wf_tr"]}
    procs["tp_min, tp_max, wf_min, wf_max"] = {"function": "min_max", "module": M, "args": ["wf_tr", *MM_NAMES]}
    outs = list(MM_NAMES) if mm else []
    if tpt is not None:
        procs["tp_0"] = {"function": "time_point_thresh", "module": M, "args": ["wf_tr", *[str(v) for v in tpt], "tp_0"]}
        outs.append("tp_0")
    if dwt is not None:
        level, part, n_out = dwt
        procs["dwt"] = {"function": "discrete_wavelet_transform", "module": M, "args": [src, level, "'h'", f"'{part}'", f"dwt({n_out}, 'f')"]}
        outs.append("dwt")
    return {"outputs": outs, "processors": procs}


def rows_oracle(wf, pz, trap, bl=None, thr=None, start="tp_max", walk=0, dwt=None):
    """{name: column} of the processors run one after the other in the float32 loop.  ``start``: 'tp_max' | 'tp_min' | a column | a number"""
    w = wf.astype(np.float32)
    if bl is not None:
        w, rc = oracle.bl_subtract(w, bl)
        assert rc == 0, ("bl_subtract", rc)
    if pz is not None:
        w, rc = (oracle.pole_zero(w, pz[1]) if pz[0] == "pole_zero" else oracle.double_pole_zero(w, *pz[1:]))
        assert rc == 0, (pz[0], rc)
    fn = {"asym_trap_filter": oracle.asym_trap_filter, "trap_filter": oracle.trap_filter, "trap_norm": oracle.trap_norm}[trap[0]]
    w2, rc = fn(w, *trap[1:])
    assert rc == 0, (trap[0], rc)
    *mm, rc = oracle.min_max(w2)
    assert rc == 0, ("min_max", rc)
    out = dict(zip(MM_NAMES, mm))
    if thr is not None:
        ts = out[start] if isinstance(start, str) else start
        out["tp_0"], rc = oracle.time_point_thresh(w2, thr, ts, walk)
        assert rc == 0, ("time_point_thresh", rc)
    if dwt is not None:
        out["dwt"], rc = oracle.dwt_haar(w, *dwt)
        assert rc == 0, ("dwt_haar", rc)
    return out


def _case(name, **kw):
    c = dict(name=name, dtype=np.int16, length=520, pz=DPZ, trap=T0_TRAP, bl=None, thr="column", dwt=None, scale=None, kernel="dsp_rows_kernel", seed=0)
    c.update(kw)
    return c


#: every shape of the rows kernel that is compared with the oracle on rows of synth_rows + a walk backward from the maximum.
#: bl: None | 'column' | 'nan_in_row_9' | a number;  thr: 'column' | a number;  kernel: what must run it
ROWS_CASES = []
for _dt in (np.float32, np.int16, np.uint16):  # the nine producers rows_produce<IN, PZ>; 65 blocks, an odd number for the two-block consumer loop
    for _pz in (PZ1, DPZ, None):
        # (unsigned rows sit 4000 counts up: their baseline is subtracted first, or pole_zero's output runs away from every threshold)
        ROWS_CASES.append(_case(f"{np.dtype(_dt).name}-{_pz[0] if _pz else 'corrected'}", dtype=_dt, pz=_pz, seed=len(ROWS_CASES) + 100,
                                bl="column" if _dt is np.uint16 else None))
#: rows shorter than the prefetch of four blocks, the two-block consumer loop and the ring
ROWS_SHORT = [_case("len16-trap_filter-8-0", length=16, trap=("trap_filter", 8, 0), seed=201),
              _case("len24-trap_filter-8-8", length=24, trap=("trap_filter", 8, 8), seed=202),
              _case("len24-asym-8-0-8", length=24, trap=("asym_trap_filter", 8, 0, 8), seed=203),
              _case("len32-trap_norm-8-8", length=32, trap=("trap_norm", 8, 8), seed=204),
              _case("len32-asym-8-8-16", length=32, trap=("asym_trap_filter", 8, 8, 16), seed=205)]
#: the ring limit: R = 312 entries, (R + 8) * 256 bytes = half a CU's LDS, is taken; one sample more of lag is the waveform VM's
ROWS_RING = [_case("ring312-trap_filter-100-104", length=2048, trap=("trap_filter", 100, 104), seed=301),
             _case("ring312-asym-9-11-284", length=2048, trap=("asym_trap_filter", 9, 11, 284), seed=302),
             _case("ring320-trap_filter-100-105", length=2048, trap=("trap_filter", 100, 105), seed=303, kernel="dsp_vm")]
ROWS_HAAR = [_case("haar7-a", length=1024, dwt=(7, "a", 8), seed=401), _case("haar7-d", length=1024, dwt=(7, "d", 8), seed=402),
             _case("haar3-a-len64", length=64, trap=("asym_trap_filter", 8, 4, 16), dwt=(3, "a", 8), seed=403)]
#: per-row and constant operands on integer rows (the producer's NaN test of the samples is compiled out for them)
ROWS_INT16 = [_case("int16-nan-baseline", bl="nan_in_row_9", seed=501), _case("int16-constant-baseline", bl=-250.5, seed=502),
              _case("int16-constant-threshold", thr=22.5, seed=503)]
ROWS_SCALED = [_case(f"float32-x{f:g}", dtype=np.float32, pz=PZ1, scale=f, seed=601) for f in (1e-42, 1e30)]
ROWS_ALL = ROWS_CASES + ROWS_SHORT + ROWS_RING + ROWS_HAAR + ROWS_INT16 + ROWS_SCALED


def rows_case(c, n=N_ROWS):
    """(recipe, input table, oracle outputs) of a case of ROWS_ALL"""
    wf, base = synth_rows(c["seed"], n, c["length"], dtype=c["dtype"])
    thr = thresholds(c["seed"] + 1, n)
    if c["scale"] is not None:
        wf, thr = scaled(wf, c["scale"]), scaled(thr, c["scale"])
    tb = {"waveform": wf}
    bl_arg = bl_val = None
    if c["bl"] in ("column", "nan_in_row_9"):
        bl_val = base + np.float32(4000 if np.dtype(c["dtype"]).kind == "u" else 0)
        if c["bl"] == "nan_in_row_9":
            bl_val[9] = np.nan
        tb["baseline"], bl_arg = bl_val, "baseline"
    elif c["bl"] is not None:
        bl_arg, bl_val = c["bl"], np.float32(c["bl"])
    if c["thr"] == "column":
        tb["thr"], thr_arg, thr_val = thr, "thr", thr
    else:
        thr_arg, thr_val = c["thr"], np.float32(c["thr"])
    recipe = rows_recipe(c["pz"], c["trap"], bl=bl_arg, tpt=(thr_arg, "tp_max", 0), dwt=c["dwt"])
    want = rows_oracle(wf, c["pz"], c["trap"], bl=bl_val, thr=thr_val, start="tp_max", walk=0, dwt=c["dwt"])
    return recipe, tb, want


#: rows_consume<TRAP, RPOW2, TPT>: the three trapezoids, a rise that is a power of two (a multiplication) or not (a division), and the
#: five walks: none, backward / forward from a column (TPT 1 / 3), backward / forward from the running extreme (TPT 2 / 4)
ROWS_TRAPS = [("trap_filter", 16, 8), ("trap_norm", 16, 8), ("trap_norm", 12, 8), ("asym_trap_filter", 8, 4, 40), ("asym_trap_filter", 12, 4, 40)]
ROWS_WALKS = {"none": None, "back-from-column": ("ts", 0), "back-from-max": ("tp_max", 0), "forward-from-column": ("ts", 1),
              "forward-from-max": ("tp_max", 1)}


def walk_case(trap, walk, n=N_ROWS, length=264):
    """(recipe, table, oracle outputs) of int16 rows through double_pole_zero, ``trap`` and the walk ROWS_WALKS[walk]"""
    seed = 900 + 10 * ROWS_TRAPS.index(trap) + list(ROWS_WALKS).index(walk)
    wf, _ = synth_rows(seed, n, length)
    tb = {"waveform": wf}
    how = ROWS_WALKS[walk]
    if how is None:
        return rows_recipe(DPZ, trap), tb, rows_oracle(wf, DPZ, trap)
    start, forward = how
    tb["thr"] = thresholds(seed + 1, n)
    if start == "ts":  # behind the step for a walk backward, ahead of it for a walk forward (the step is at 0.45 .. 0.55 of the row)
        rng = np.random.default_rng(seed + 2)
        tb["ts"] = (rng.integers(3 * length // 4, length, n) if not forward else rng.integers(0, length // 4, n)).astype(np.float32)
    want = rows_oracle(wf, DPZ, trap, thr=tb["thr"], start=tb["ts"] if start == "ts" else start, walk=forward)
    return rows_recipe(DPZ, trap, tpt=("thr", start, forward)), tb, want


#: the STOP build: each type of row, each trapezoid
STOP_CASES = [(np.float32, T0_TRAP), (np.int16, T0_TRAP), (np.uint16, T0_TRAP)] + [(np.float32, t) for t in ROWS_TRAPS]
STOP_NAN_ROW = 20


def stop_case(dtype=np.float32, trap=T0_TRAP, n=200, length=1024):
    """The STOP build: rows another program corrected already (the LOAD's promise: free of NaN or NaN throughout), no pole-zero step, a
    walk backward from a known start column and no other output.  Four groups of rows: (0) starts 0, 7, 8 and NaN among ordinary ones,
    (1) NaN starts only, (2) one start in the last sample, (3) a partial group.  float32 rows are what pole_zero wrote, row STOP_NAN_ROW
    NaN throughout.  Returns (recipe, table, oracle tp_0)."""
    wf, _ = synth_rows(701, n, length, dtype=dtype)
    if np.dtype(dtype) == np.float32:
        wf[STOP_NAN_ROW, 333] = np.nan  # pole_zero makes the whole row NaN: the promise's other half
        wf, rc = oracle.pole_zero(wf, PZ1[1])
        assert rc == 0 and np.isnan(wf[STOP_NAN_ROW]).all() and not np.isnan(np.delete(wf, STOP_NAN_ROW, axis=0)).any()
    rng = np.random.default_rng(702)
    ts = rng.integers(length // 2, length // 2 + 200, n).astype(np.float32)  # behind the step (at 0.45 .. 0.55 of the row)
    ts[[1, 2, 3, 4]] = (0, 7, 8, np.nan)
    ts[64:128] = np.nan
    ts[130] = length - 1
    thr = thresholds(703, n)
    recipe = rows_recipe(None, trap, tpt=("thr", "ts", 0), mm=False)
    want = rows_oracle(wf, None, trap, thr=thr, start=ts, walk=0)
    return recipe, {"waveform": wf, "thr": thr, "ts": ts}, want["tp_0"]


def set_load_promise(program):
    """the LOAD of a program compiled from a recipe, with the promise a stage's LOAD carries (DSP_OP_LOAD ip[2] & 1: every row is free of
    NaN or NaN throughout -- what pole_zero writes)"""
    opcode, dst, src, io, ip, sp = program.ops[0]
    ip = tuple(ip) + (0,) * (3 - len(ip))
    program.ops[0] = (opcode, dst, src, io, (ip[0], ip[1], ip[2] | 1), sp)
    return program


# ------------------------------------------------------------------------------------------------------------------------------------
# fit kernel: dsp_linear_slope_fit_rows
# ------------------------------------------------------------------------------------------------------------------------------------
FIT_SLOPE_SCALE, FIT_INTERCEPT_SCALE = 0.05, 4000.0  # the largest slope and step of fit_rows: what the 2e-6 bar is relative to


def fit_rows(n, length, dtype, seed, factor=1):
    """a noisy sloped baseline with a decaying step in the second half (the generator of test_gpu_fit_rows), times ``factor``"""
    rng = np.random.default_rng(seed)
    w = 3000 + 6 * rng.standard_normal((n, length)) + rng.uniform(-0.05, 0.05, (n, 1)) * np.arange(length)[None, :]
    w[:, length // 2:] += rng.uniform(50, 4000, (n, 1)) * np.exp(-np.arange(length - length // 2) / 800.0)[None, :]
    return (w * factor).astype(dtype)


def fit_oracle(w, fits, sub, mode, tau, ft):
    """(n_fits, 4, n) of bl_subtract | numpy.subtract -> pole_zero -> linear_slope_fit on each window, in the loop of type ``ft``"""
    y = w.astype(ft)
    if mode == 1:
        y, rc = oracle.bl_subtract(y, sub)
        assert rc == 0
    elif mode == 2:
        y = (y - (np.asarray(sub, dtype=ft)[:, None] if isinstance(sub, np.ndarray) else ft(sub))).astype(ft)
    z = None
    if tau is not None:
        z, rc = oracle.pole_zero(y, tau)
        assert rc == 0
    res = []
    for stage, first, count in fits:
        *o, rc = oracle.linear_slope_fit(np.ascontiguousarray((z if stage else y)[:, first:first + count]))
        assert rc == 0, ((stage, first, count), rc)
        res.append(np.stack(o))
    return np.stack(res)


#: (rows' type, loop's type): int16 is the production type (8 samples per 16-byte load); float32 and uint32 rows in the float64 loop
FIT_TYPES = [(np.int16, np.float32), (np.float32, np.float64), (np.uint32, np.float64)]
#: 16-bit rows in the float64 loop: no recipe asks for it, the C entry point takes it
FIT_TYPES_F64_16BIT = [(np.int16, np.float64), (np.uint16, np.float64)]
#: windows that start or end on an edge of the kernel's 64-sample tiles, of 2 and 3 samples across one; (stage, first, count)
FIT_TILE_EDGE_WINDOWS = [(0, 0, 64), (0, 64, 64), (0, 63, 2), (0, 63, 3), (0, 64, 65), (1, 128, 64)]
#: the Ge recipe's fits: the baseline at the start, nothing for 400 samples (the pole-zero state carried), the corrected tail
FIT_PRODUCTION_WINDOWS = [(0, 0, 300), (1, 700, 300)]
FIT_TAU = 271.25
