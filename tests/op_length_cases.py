"""Every waveform op of the interpreter (dsp_vm.hip) at the row lengths where its LDS layout changes: the cases and their oracle-side
expectations for tests/test_gpu_op_lengths.py (the device) and tests/test_op_length_cases_cpu.py (do the cases say something? -- the
planner and the oracle alone).  Nothing here needs a GPU; every row comes from a seed.

The interpreter keeps a row of ``n`` samples as 64 lane chunks of ``C = 16 * ceil(n / 1024)`` samples at a pitch of ``C + 1``
(dsp_plan.cpp, ``chunk``).  A partial last chunk and the chunks of lanes that own nothing hold zeros that are only "kept finite"; the
slot reads as zeros beyond its last sample only where ``n == 64 * C``; rows whose stride keeps 16-byte alignment go through vector loads
and stores, the others sample by sample.  ``LENGTHS`` walks those boundaries, and the rows (``batch``) are made so that a pad taken for a
sample shows: all-negative and all-positive rows, extremes in the first and the last sample, a step inside the last occupied chunk, NaN
in the first or the last sample alone.

A ``Case`` is one op with one set of parameters at one length in one row type, the parameters made from the length by rule (``OPS``).  Its
expectation is what ``oracle.*`` returns for the same bits in the loop's type -- or the error the oracle's return code stands for.  It can
be run in three forms: ``call`` (A: the processor of dspeed_amd.processors, default routing), ``recipe("B")`` (a recipe kept whole on the
interpreter by vm_row_loop_cases.switches, the op reading the loaded rows) and ``recipe("C")`` (the op reads ``wf_c = waveform + 0``, which
a numpy.amax reads as well; an output waveform is stored and feeds a min_max)."""
import functools

import numpy as np

import oracle
from vm_row_loop_cases import switches  # noqa: F401  (the GPU and CPU tests take it from here)

M = "dspeed.processors"
#: the interpreter's own boundaries ...
LAYOUT_LENGTHS = (1, 2, 3, 5, 15, 16, 17, 31, 33, 63, 64, 65, 1009, 1023, 1024, 1025, 2047, 2049, 3073)
#: ... and both sides of the one admission flip of form A that they do not hold (test_op_length_cases_cpu.py scans for them): a FIR of 64
#: taps or more on float32 / int16 rows goes to the float16 matrix-core kernel where the row length is a multiple of 8 (64, 1024), to
#: dsp_fir_store_kernel where it is 4 more than one -- 68 is the first such length -- and to the interpreter everywhere else
ROUTE_LENGTHS = (67, 68, 69)
LENGTHS = tuple(sorted(LAYOUT_LENGTHS + ROUTE_LENGTHS))
TAGS = ("f32", "f64", "i16")
ROW_TYPES = {"f32": np.float32, "f64": np.float64, "i16": np.int16}
KINDS = ("noise", "negative", "positive", "max-first-min-last", "min-first-max-last", "constant", "step-in-last-chunk", "pulse", "nan-last",
         "nan-first")
SEEDS = 7
ROWS = len(KINDS) * SEEDS  # 70: more than the 64 rows of one wavefront of the lane-per-row routes
ONE_SIGNED = ("negative", "positive")
CLASSES = ("single partial chunk", "chunk-exact", "one sample into the next chunk", "len == 64 * C", "C just grown", "odd stride",
           "partial last chunk")

FATAL, ZERODIV = "DSPFatal", "ZeroDivisionError"


def chunk(n):
    """the planner's lane chunk of a slot of n samples (dsp_plan.cpp: "int C = (len + 63) / 64; C = ((C + 15) / 16) * 16")"""
    c = (n + 63) // 64
    return ((c + 15) // 16) * 16


def last_chunk_start(n):
    """the first sample of the last lane chunk that holds a sample"""
    return ((n - 1) // chunk(n)) * chunk(n)


def classes(n):
    """the names of CLASSES that the length belongs to"""
    c = chunk(n)
    out = []
    if n < c:
        out.append("single partial chunk")
    if n % c == 0 and n != 64 * c:
        out.append("chunk-exact")
    if n % c == 1 and n > 1:
        out.append("one sample into the next chunk")
    if n == 64 * c:
        out.append("len == 64 * C")
    if n > 1 and chunk(n - 1) < c:
        out.append("C just grown")
    if n > c and n % c > 1:
        out.append("partial last chunk")
    if n % 4:  # (a float32 row stride that is no multiple of 16 bytes: no vector loads or stores in any of the three row types)
        out.append("odd stride")
    return tuple(out)


def loop_type(tag):
    return np.dtype(np.float64 if tag == "f64" else np.float32)


def error_of(rc):
    """what the device raises for the oracle's return code (dspeed_amd._lib.check; golden_util.zerodiv names the same rule)"""
    return None if rc == 0 else (ZERODIV if oracle.E_NAMES.get(rc) == "ZERODIV" else FATAL)


# ------------------------------------------------------------------------------------------------------------------------------------
# rows
# ------------------------------------------------------------------------------------------------------------------------------------
def _row(kind, n, seed):
    rng = np.random.default_rng([n, KINDS.index(kind), seed])
    i = np.arange(n, dtype=np.float64)
    if kind in ("noise", "nan-last", "nan-first"):
        return 100.0 * rng.standard_normal(n)
    if kind == "negative":
        return -3000.0 + rng.uniform(-50, 50, n)
    if kind == "positive":
        return 3000.0 + rng.uniform(-50, 50, n)
    if kind in ("max-first-min-last", "min-first-max-last"):
        w = np.clip(100.0 * rng.standard_normal(n), -300, 300)
        hi, lo = 1000.0 + 10 * seed, -1000.0 - 10 * seed
        w[0], w[n - 1] = (hi, lo) if kind == "max-first-min-last" else (lo, hi)  # (one sample: the second assignment stands)
        return w
    if kind == "constant":
        return np.full(n, 500.0 * (seed - 3) + 7.0)
    if kind == "step-in-last-chunk":
        onset = int(rng.integers(last_chunk_start(n), n))
        return -200.0 + 5.0 * rng.standard_normal(n) + 1000.0 * (i >= onset)
    assert kind == "pulse"
    t0 = np.floor(rng.uniform(0.3, 0.6) * n)
    d = i - t0
    return rng.uniform(-100, 100) + rng.uniform(500, 5000) * np.exp(-np.clip(d, 0, None) / (n / 2.0)) * (d >= 0) + 5.0 * rng.standard_normal(n)


@functools.lru_cache(maxsize=None)
def batch(n, tag):
    """the ROWS rows of length n in the row type of ``tag``: row r is of kind r % 10, seed r // 10.  The int16 batch holds the type's extremes
    where the float batches hold their NaN"""
    x = np.stack([_row(KINDS[r % len(KINDS)], n, r // len(KINDS)) for r in range(ROWS)])
    kind = kinds()
    if tag == "i16":
        w = np.rint(x).astype(np.int16)
        w[kind == KINDS.index("nan-last"), n - 1] = np.iinfo(np.int16).max
        w[kind == KINDS.index("nan-first"), 0] = np.iinfo(np.int16).min
    else:
        w = x.astype(ROW_TYPES[tag])
        w[kind == KINDS.index("nan-last"), n - 1] = np.nan
        w[kind == KINDS.index("nan-first"), 0] = np.nan
    w.setflags(write=False)
    return w


def kinds():
    return np.arange(ROWS) % len(KINDS)


def seeds():
    return np.arange(ROWS) // len(KINDS)


def is_kind(*names):
    return np.isin(kinds(), [KINDS.index(k) for k in names])


def in_loop(w, tag):
    """the rows as the loop sees them"""
    return np.ascontiguousarray(w, dtype=loop_type(tag))


def finite_rows(w):
    return np.isfinite(np.asarray(w, dtype=np.float64)).all(axis=1)


# ------------------------------------------------------------------------------------------------------------------------------------
# a case
# ------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """``op``: the name in OPS; ``name``: op and parameters; ``cols``: name -> per-row column in the loop's type; ``outs``: [(name, length or
    0 for a value per row)]; ``oracle(w, cols)`` -> (outputs..., rc); ``call(P, w, cols)``: form A, or None where the op is no processor;
    ``proc(src, outs)``: the recipe entry that reads the variable ``src`` (a processor description or an expression); ``bars``: one per
    output -- 'exact', ('peak', 'filter' | 'dpz'), ('fir', sum |k|), ('rtol', r), ('atol_in', a), ('fit', 'slope' | 'icpt')"""

    def __init__(self, op, name, n, tag, cols, outs, oracle_fn, call, proc, bars, walk=False, pad_oracle=None):
        self.op, self.name, self.n, self.tag, self.cols, self.outs = op, name, n, tag, cols, outs
        self._oracle, self.call, self._proc, self.bars, self.walk, self.pad_oracle = oracle_fn, call, proc, bars, walk, pad_oracle
        self.ft = loop_type(tag)
        self.id = f"{name}-{n}-{tag}"

    @property
    def rows(self):
        return batch(self.n, self.tag)

    @functools.lru_cache(maxsize=None)
    def expect(self):
        """(outputs as a list of arrays, error): the oracle on the rows in the loop's type"""
        with np.errstate(all="ignore"):
            *out, rc = self._oracle(in_loop(self.rows, self.tag), self.cols)
        return [np.asarray(o) for o in out], error_of(rc)

    def recipe(self, form):
        """(recipe, input table, names of the op's outputs, extra outputs: {'m': amax of wf_c, 'mm': min_max of the op's first waveform})"""
        assert form in "BC"
        register_taps_loader()
        src = "waveform" if form == "B" else "wf_c"
        names = [o[0] for o in self.outs]
        decl = [f"{k}({length}, '{'d' if self.tag == 'f64' else 'f'}')" if length else k for k, length in self.outs]
        procs, extra = {}, {}
        if form == "C":
            procs["wf_c"] = "waveform + 0"
            procs["c_max"] = {"function": "amax", "module": "numpy", "args": ["wf_c", 1, "c_max"]}
            extra["m"] = "c_max"
        procs[", ".join(names)] = self._proc(src, decl)
        if form == "C" and self.outs[0][1]:
            mm = ["o_tlo", "o_thi", "o_lo", "o_hi"]
            procs[", ".join(mm)] = {"function": "min_max", "module": M, "args": [names[0], *mm]}
            extra["mm"] = mm
        outputs = names + ([extra["m"]] if "m" in extra else []) + extra.get("mm", [])
        table = {"waveform": self.rows, **self.cols}
        return {"outputs": outputs, "processors": procs}, table, names, extra


def _p(fn, *args, module=M):
    return {"function": fn, "module": module, "args": list(args)}


def _lit(v):
    """a constant as a recipe writes it: the shortest text that reads back as the same float64"""
    return repr(float(v))


def _col(values, tag):
    a = np.asarray(values, dtype=loop_type(tag))
    a.setflags(write=False)
    return a


def _outbuf(n_rows, length, tag):
    return np.empty((n_rows, length), dtype=loop_type(tag))


# ------------------------------------------------------------------------------------------------------------------------------------
# the ops: parameters by rule from n
# ------------------------------------------------------------------------------------------------------------------------------------
def trap_params(n):
    """rise, flat, fall: about n / 8, n / 16 and n / 5, at least 1"""
    return max(1, n // 8), max(1, n // 16), max(1, n // 5)


def _c_bl_subtract(n, tag):
    bl = _col(np.random.default_rng([n, 101]).uniform(-500, 500, ROWS), tag)
    return [Case("bl_subtract", "bl_subtract", n, tag, {"bl": bl}, [("o", n)], lambda w, c: oracle.bl_subtract(w, c["bl"]),
                 lambda P, w, c: [P.bl_subtract(w, c["bl"])], lambda src, o: f"{M}.bl_subtract({src}, bl, {o[0]})", ["exact"])]


def _c_pole_zero(n, tag):
    tau = max(1.5, n / 3.0)
    return [Case("pole_zero", "pole_zero", n, tag, {}, [("o", n)], lambda w, c: oracle.pole_zero(w, tau), lambda P, w, c: [P.pole_zero(w, tau)],
                 lambda src, o: _p("pole_zero", src, _lit(tau), o[0]), [("peak", "filter")])]


def _c_double_pole_zero(n, tag):
    t1, t2, frac = max(2.0, n / 3.0), max(1.25, n / 40.0), 0.02
    return [Case("double_pole_zero", "double_pole_zero", n, tag, {}, [("o", n)], lambda w, c: oracle.double_pole_zero(w, t1, t2, frac),
                 lambda P, w, c: [P.double_pole_zero(w, t1, t2, frac)], lambda src, o: _p("double_pole_zero", src, _lit(t1), _lit(t2), _lit(frac), o[0]),
                 [("peak", "dpz")])]


def _c_traps(fn):
    def make(n, tag):
        r, f, fall = trap_params(n)
        a = (r, f, fall) if fn == "asym_trap_filter" else (r, f)
        return [Case(fn, fn, n, tag, {}, [("o", n)], lambda w, c: getattr(oracle, fn)(w, *a), lambda P, w, c: [getattr(P, fn)(w, *a)],
                     lambda src, o: _p(fn, src, *map(str, a), o[0]), [("peak", "filter")])]
    return make


def pickoff_times(n, whole):
    """a time per row: 0, n - 1, the last chunk's first sample and (unless ``whole``) fractional times inside the last chunk and the row"""
    lc = last_chunk_start(n)
    rng = np.random.default_rng([n, 102])
    t = np.array([0.0, n - 1.0, float(lc), lc + 0.25, n - 1.5, lc + 0.5 * (n - 1 - lc), 0.75])[np.arange(ROWS) % 7]
    t = np.where(np.arange(ROWS) >= 49, rng.uniform(0, n - 1, ROWS), t)
    t = np.clip(t, 0, n - 1)
    return np.floor(t) if whole else t


def _c_fixed_time_pickoff(n, tag):
    out = []
    for mode in "nfclhsi":
        t = _col(pickoff_times(n, mode == "i"), tag)
        bar = ("rtol", 1e-13) if (mode == "h" and tag == "f64") else "exact"  # (test_fixed_time_pickoff_golden: x * (x * x) against pow)
        out.append(Case("fixed_time_pickoff", f"fixed_time_pickoff-{mode}", n, tag, {"t_in": t}, [("o", 0)],
                        lambda w, c, mode=mode: oracle.fixed_time_pickoff(w, c["t_in"], mode),
                        lambda P, w, c, mode=mode: [P.fixed_time_pickoff(w, c["t_in"], ord(mode))],
                        lambda src, o, mode=mode: _p("fixed_time_pickoff", src, "t_in", f"'{mode}'", o[0]), [bar]))
    return out


def walk_columns(n, tag, forward):
    """threshold and start of every row.  Start: seed % 3 == 0 the end the walk leaves from (0 forwards, n - 1 backwards), 1 the other end,
    2 the row's maximum.  Threshold: half way between the row's extremes -- below 8 samples half way between the two samples at the walk's
    start --; for the one-signed kinds half way between the row and 0: no sample crosses it, a pad read as a sample would"""
    w = in_loop(batch(n, tag), tag).astype(np.float64)
    fin = np.where(np.isnan(w), 0.0, w)
    lo, hi = fin.min(axis=1), fin.max(axis=1)
    thr = 0.5 * (lo + hi)
    if 2 <= n < 8:
        thr = 0.5 * (fin[:, 0] + fin[:, 1]) if forward else 0.5 * (fin[:, n - 2] + fin[:, n - 1])
    signed = is_kind(*ONE_SIGNED)
    thr = np.where(signed, 0.5 * np.where(hi < 0, hi, lo), thr)
    leave, other = (0.0, n - 1.0) if forward else (n - 1.0, 0.0)
    start = np.select([seeds() % 3 == 0, seeds() % 3 == 1], [leave, other], fin.argmax(axis=1).astype(np.float64))
    start = np.where(signed, leave, start)  # (the one-signed rows walk the whole row, and beyond it if the kernel lets them)
    return _col(thr, tag), _col(start, tag)


def _c_time_point_thresh(n, tag):
    out = []
    for fwd in (1, 0):
        thr, ts = walk_columns(n, tag, bool(fwd))
        out.append(Case("time_point_thresh", f"time_point_thresh-walk{fwd}", n, tag, {"thr": thr, "t_start": ts}, [("o", 0)],
                        lambda w, c, fwd=fwd: oracle.time_point_thresh(w, c["thr"], c["t_start"], fwd),
                        lambda P, w, c, fwd=fwd: [P.time_point_thresh(w, c["thr"], c["t_start"], fwd)],
                        lambda src, o, fwd=fwd: f"{M}.time_point_thresh({src}, thr, t_start, {fwd}, {o[0]})", ["exact"], walk=True,
                        # (the backward walk leaves the row at sample 0, where no pad lies)
                        pad_oracle=(lambda w, c: oracle.time_point_thresh(w, c["thr"], c["t_start"], 1)) if fwd else None))
    return out


def _c_interpolated_time_point_thresh(n, tag):
    out = []
    for fwd in (1, 0):
        thr, ts = walk_columns(n, tag, bool(fwd))
        for mode in "ibcafrnl":
            out.append(Case("interpolated_time_point_thresh", f"interpolated_time_point_thresh-walk{fwd}-{mode}", n, tag, {"thr": thr, "t_start": ts}, [("o", 0)],
                            lambda w, c, fwd=fwd, mode=mode: oracle.interpolated_time_point_thresh(w, c["thr"], c["t_start"], fwd, mode),
                            lambda P, w, c, fwd=fwd, mode=mode: [P.interpolated_time_point_thresh(w, c["thr"], c["t_start"], fwd, ord(mode))],
                            lambda src, o, fwd=fwd, mode=mode: f"{M}.interpolated_time_point_thresh({src}, thr, t_start, {fwd}, '{mode}', {o[0]})",
                            ["exact"], walk=True))
    return out


def _c_min_max(n, tag):
    names = [("t_lo", 0), ("t_hi", 0), ("a_lo", 0), ("a_hi", 0)]
    return [Case("min_max", "min_max", n, tag, {}, names, lambda w, c: oracle.min_max(w), lambda P, w, c: list(P.min_max(w)),
                 lambda src, o: _p("min_max", src, *o), ["exact"] * 4, pad_oracle=lambda w, c: oracle.min_max(w))]


def _c_min_max_norm(n, tag):
    w = in_loop(batch(n, tag), tag)
    _t0, _t1, lo, hi, rc = oracle.min_max(w)
    assert rc == 0
    cols = {"a_lo": _col(lo, tag), "a_hi": _col(hi, tag)}
    return [Case("min_max_norm", "min_max_norm", n, tag, cols, [("o", n)], lambda w, c: oracle.min_max_norm(w, c["a_lo"], c["a_hi"]),
                 lambda P, w, c: [P.min_max_norm(w, c["a_lo"], c["a_hi"])], lambda src, o: _p("min_max_norm", src, "a_lo", "a_hi", o[0]), ["exact"])]


def _amax(w, c):
    with np.errstate(all="ignore"):
        return np.max(w, axis=1), 0  # (numpy.amax: a NaN wins)


def _c_amax(n, tag):
    return [Case("amax", "amax", n, tag, {}, [("o", 0)], _amax, None, lambda src, o: _p("amax", src, 1, o[0], module="numpy"), ["exact"], pad_oracle=_amax)]


def mean_below_thresholds(n, tag):
    """above 0 on the all-negative rows (every sample lies below, a zero pad would too), below the rows on the all-positive ones (nothing
    lies below, a zero pad would), the row's median elsewhere"""
    w = in_loop(batch(n, tag), tag).astype(np.float64)
    thr = np.median(np.where(np.isnan(w), 0.0, w), axis=1) + 0.5
    thr = np.where(is_kind("negative"), 100.0, np.where(is_kind("positive"), 1000.0, thr))
    return _col(thr, tag)


def _c_mean_below_threshold(n, tag):
    bar = ("rtol", 1e-13) if tag == "f64" else "exact"  # (test_mean_below_threshold_golden: float64 partial sums in another order)
    fn = lambda w, c: oracle.mean_below_threshold(w, c["thr"])  # noqa: E731
    return [Case("mean_below_threshold", "mean_below_threshold", n, tag, {"thr": mean_below_thresholds(n, tag)}, [("o", 0)], fn,
                 lambda P, w, c: [P.mean_below_threshold(w, c["thr"])], lambda src, o: f"{M}.mean_below_threshold({src}, thr, {o[0]})", [bar], pad_oracle=fn)]


def _c_linear_slope_fit(n, tag):
    names = [("f_mean", 0), ("f_std", 0), ("f_slope", 0), ("f_icpt", 0)]
    fn = lambda w, c: oracle.linear_slope_fit(w)  # noqa: E731
    return [Case("linear_slope_fit", "linear_slope_fit", n, tag, {}, names, fn, lambda P, w, c: list(P.linear_slope_fit(w)),
                 lambda src, o: _p("linear_slope_fit", src, *o), ["exact", "exact", ("fit", "slope"), ("fit", "icpt")], pad_oracle=fn)]


def window_length(n):
    return max(1, n // 2)


def window_starts(n):
    """a start per row: partly before the row, inside it (both ends, a fractional one), partly beyond it"""
    m = window_length(n)
    return np.array([-(m // 2) - 1.0, 0.0, float(n - m), n - m - 0.5, n - m // 2 - 0.0, 0.5 * (n - m), 1.0])[np.arange(ROWS) % 7]


def _c_windower(n, tag):
    m = window_length(n)
    return [Case("windower", "windower", n, tag, {"t0": _col(window_starts(n), tag)}, [("o", m)], lambda w, c: oracle.windower(w, c["t0"], m),
                 lambda P, w, c: [P.windower(w, c["t0"], _outbuf(len(w), m, tag))], lambda src, o: f"{M}.windower({src}, t0, {o[0]})", ["exact"])]


def _c_avg_current(n, tag):
    L = max(1, n // 10)
    m = max(n - L, 1)
    return [Case("avg_current", "avg_current", n, tag, {}, [("o", m)], lambda w, c: oracle.avg_current(w, L, m),
                 lambda P, w, c: [P.avg_current(w, L, _outbuf(len(w), m, tag))], lambda src, o: f"{M}.avg_current({src}, {L}, {o[0]})", ["exact"])]


UPSAMPLE_16_MAX = 1025  # (16 x 1025 float64 samples and the row beside them fit a wavefront's LDS; 16 x 2047 do not)


def _c_upsampler(n, tag):
    out = []
    for up in (2, 16):
        if up == 16 and n > UPSAMPLE_16_MAX:
            continue
        m = n * up
        out.append(Case("upsampler", f"upsampler-x{up}", n, tag, {}, [("o", m)], lambda w, c, up=up, m=m: oracle.upsampler(w, up, m),
                        lambda P, w, c, up=up, m=m: [P.upsampler(w, up, _outbuf(len(w), m, tag))],
                        lambda src, o, up=up: f"{M}.upsampler({src}, {up}, {o[0]})", ["exact"]))
    return out


def _c_moving_window_multi(n, tag):
    L = max(1, n // 10)
    out = []
    for num, typ in ((1, 0), (3, 0), (1, 1), (3, 1)):
        out.append(Case("moving_window_multi", f"moving_window_multi-{num}-type{typ}", n, tag, {}, [("o", n)],
                        lambda w, c, num=num, typ=typ: oracle.moving_window_multi(w, L, num, typ),
                        lambda P, w, c, num=num, typ=typ: [P.moving_window_multi(w, L, num, typ)],
                        lambda src, o, num=num, typ=typ: f"{M}.moving_window_multi({src}, {L}, {num}, {typ}, {o[0]})", [("peak", "filter")]))
    return out


def trap_pickoff_times(n):
    """whole samples: the first at which both windows lie in the row, the last sample, the last chunk's first sample, one before the first
    that fits and one past the row (NaN results), and seeded ones between"""
    r, f, _ = trap_params(n)
    first = 2 * r + f - 1
    rng = np.random.default_rng([n, 103])
    t = np.array([first, n - 1, max(first, last_chunk_start(n)), first - 1, n, 0, 0], dtype=np.float64)[np.arange(ROWS) % 7]
    between = np.floor(rng.uniform(first, max(first + 1, n), ROWS))
    return np.where(np.arange(ROWS) % 7 >= 5, np.minimum(between, n - 1), t)


def _c_trap_pickoff(n, tag):
    r, f, _ = trap_params(n)
    bar = ("atol_in", 1e-12) if tag == "f64" else "exact"  # (test_windows_golden: float64 partial sums in another order)
    return [Case("trap_pickoff", "trap_pickoff", n, tag, {"t_pk": _col(trap_pickoff_times(n), tag)}, [("o", 0)],
                 lambda w, c: oracle.trap_pickoff(w, r, f, c["t_pk"]), lambda P, w, c: [P.trap_pickoff(w, r, f, c["t_pk"])],
                 lambda src, o: _p("trap_pickoff", src, str(r), str(f), "t_pk", o[0]), [bar])]


def _c_dwt(n, tag):
    out = []
    for level in (1, 2, 3):
        m = n
        for _ in range(level):
            m = (m + 1) // 2
        for part in "ad":
            out.append(Case("discrete_wavelet_transform", f"discrete_wavelet_transform-{level}{part}", n, tag, {}, [("o", m)],
                            lambda w, c, level=level, part=part, m=m: oracle.dwt_haar(w, level, part, m),
                            lambda P, w, c, level=level, part=part, m=m: [P.discrete_wavelet_transform(w, level, ord("h"), ord(part), _outbuf(len(w), m, tag))],
                            lambda src, o, level=level, part=part: _p("discrete_wavelet_transform", src, level, "'h'", f"'{part}'", o[0]), ["exact"]))
    return out


def fir_taps(m):
    """m seeded taps, multiples of 1/16 in [-1, 1] without 0: the same numbers in float32 and float64"""
    rng = np.random.default_rng([m, 104])
    k = rng.integers(1, 17, m) * rng.choice([-1, 1], m)
    return k / 16.0


TAPS_FILE = "mem:op_length_taps"  # (a recipe reads its taps with loadlh5(TAPS_FILE, '<m>'): float32, as a kernel file holds them)


def _taps_loader(file, path):
    return fir_taps(int(path)).astype(np.float32) if file == TAPS_FILE else None


def register_taps_loader():
    from dspeed_amd import lgdo_io

    if _taps_loader not in lgdo_io.CONSTANT_LOADERS:
        lgdo_io.CONSTANT_LOADERS.append(_taps_loader)


def fir_lengths(n):
    return sorted({1, 2, 16, 17, min(n, 133)})


def _c_convolve_wf(n, tag):
    out = []
    for m in fir_lengths(n):
        k = fir_taps(m)
        for mode, p in (("f", n + m - 1), ("v", max(n - m + 1, 1)), ("s", n)):
            out.append(Case("convolve_wf", f"convolve_wf-{mode}-{m}taps", n, tag, {}, [("o", p)],
                            lambda w, c, k=k, mode=mode, p=p: oracle.convolve_wf(w, k.astype(w.dtype), mode, p),
                            lambda P, w, c, k=k, mode=mode, p=p: [P.convolve_wf(w, k.astype(loop_type(tag)), ord(mode), _outbuf(len(w), p, tag))],
                            lambda src, o, m=m, mode=mode: _p("convolve_wf", src, f"loadlh5('{TAPS_FILE}', '{m}')", f"'{mode}'", o[0]),
                            [("fir", float(np.abs(k).sum()))]))
    return out


def slices(n):
    """constant slices with step 1, 3 and -1 that touch both ends of the row"""
    out = [("rev", slice(None, None, -1), "[::-1]"), ("step3", slice(0, n, 3), f"[0:{n}:3]"), ("step3-last", slice((n - 1) % 3, n, 3), f"[{(n - 1) % 3}:{n}:3]")]
    if n >= 2:
        out += [("tail", slice(1, n), f"[1:{n}]"), ("head", slice(0, n - 1), f"[0:{n - 1}]")]
    return out


def _c_slice(n, tag):
    out = []
    for name, sl, text in slices(n):
        m = len(range(n)[sl])
        out.append(Case("slice", f"slice-{name}", n, tag, {}, [("o", m)], lambda w, c, sl=sl: (np.ascontiguousarray(w[:, sl]), 0), None,
                        lambda src, o, text=text: f"{src}{text}", ["exact"]))
    return out


def _c_where(n, tag):
    return [Case("where", "where", n, tag, {}, [("o", n)], lambda w, c: (np.where(w < 0, w.dtype.type(0), w), 0), None,
                 lambda src, o: f"where({src} < 0, 0, {src})", ["exact"])]


OPS = {
    "bl_subtract": _c_bl_subtract, "pole_zero": _c_pole_zero, "double_pole_zero": _c_double_pole_zero, "trap_filter": _c_traps("trap_filter"),
    "trap_norm": _c_traps("trap_norm"), "asym_trap_filter": _c_traps("asym_trap_filter"), "fixed_time_pickoff": _c_fixed_time_pickoff,
    "time_point_thresh": _c_time_point_thresh, "interpolated_time_point_thresh": _c_interpolated_time_point_thresh, "min_max": _c_min_max,
    "min_max_norm": _c_min_max_norm, "amax": _c_amax, "mean_below_threshold": _c_mean_below_threshold, "linear_slope_fit": _c_linear_slope_fit,
    "windower": _c_windower, "avg_current": _c_avg_current, "upsampler": _c_upsampler, "moving_window_multi": _c_moving_window_multi,
    "trap_pickoff": _c_trap_pickoff, "discrete_wavelet_transform": _c_dwt, "convolve_wf": _c_convolve_wf, "slice": _c_slice, "where": _c_where}

#: the ops whose result a zero pad taken for a sample changes on a one-signed row (the discrimination check of the CPU test)
PAD_SENSITIVE = ("min_max", "amax", "mean_below_threshold", "time_point_thresh", "linear_slope_fit")

#: the shortest row the oracle takes with the parameters the rules above give: read off its return codes (test_op_length_cases_cpu.py
#: holds the table against them).  Below it the case's expectation is the oracle's error
MIN_LENGTH = {
    "bl_subtract": 1, "pole_zero": 1, "double_pole_zero": 4, "trap_filter": 3, "trap_norm": 3, "asym_trap_filter": 3, "fixed_time_pickoff": 1,
    "time_point_thresh": 1, "interpolated_time_point_thresh": 1, "min_max": 1, "min_max_norm": 1, "amax": 1, "mean_below_threshold": 1,
    "linear_slope_fit": 2, "windower": 2, "avg_current": 2, "upsampler": 1, "moving_window_multi": 2, "trap_pickoff": 3,
    "discrete_wavelet_transform": 1, "convolve_wf": 1, "slice": 1, "where": 1}

#: a walk needs a pair of samples to cross between; the backward walk of interpolated_time_point_thresh stops at sample 2
#: (range(int(t_start), 1, -1)): below these lengths no row can cross, and the crossing condition of the CPU test starts at them
WALK_CAN_CROSS = {"time_point_thresh-walk1": 2, "time_point_thresh-walk0": 2, "interpolated_time_point_thresh-walk1": 2,
                  "interpolated_time_point_thresh-walk0": 3}


#: cases whose device result and oracle expectation lie just further apart than the bar although the device is no further from a
#: higher-precision evaluation of the same rows than the oracle is (profiles/r10_op_lengths.md has the figures): the GPU module runs them
#: in a test of their own, at the same bar, marked xfail(strict=True)
OVER_THE_BAR = {
    "moving_window_multi-3-type1-1025-f32": "row 22: 1.14e-6 of the peak between device and oracle (bar 1e-6); against the float64 recurrence the device "
                                            "is off by 1.32e-6 in that row, the oracle by 2.30e-6 (worst row of the batch: 3.05e-6 both)",
    "moving_window_multi-3-type0-2047-f32": "row 22: 1.06e-6 of the peak between device and oracle (bar 1e-6); against the float64 recurrence the worst "
                                            "row of the batch is off by 3.02e-6 on the device, by 3.17e-6 in the oracle (row 22: 2.30e-6 and 1.40e-6)",
    "mean_below_threshold-2047-f64": "row 37: the mean is -0.0078 of samples of mean magnitude 131, the sum cancels 17 000-fold; device and oracle differ "
                                     "by 2.6e-12 of it (bar: rtol 1e-13); against the exact sum (math.fsum) the device is off by 2.7e-13, the oracle by 2.4e-12",
}


def min_length(case):
    """MIN_LENGTH of the case's op; a FIR needs a row as long as its taps (ORC_E_CONV_LONG)"""
    if case.op == "convolve_wf":
        return int(case.name.split("-")[2][:-4])
    return MIN_LENGTH[case.op]


@functools.lru_cache(maxsize=None)
def cases(op, n, tag):
    return tuple(OPS[op](n, tag))


def padded(w, n):
    """the rows extended with zeros to 64 * C samples: what a kernel would see that took the pads for samples"""
    return np.concatenate([w, np.zeros((len(w), 64 * chunk(n) - n), dtype=w.dtype)], axis=1)


# ------------------------------------------------------------------------------------------------------------------------------------
# form A's program (dsp_gufuncs.cpp, restated): what the processor call hands to the planner
# ------------------------------------------------------------------------------------------------------------------------------------
def processor_program(case):
    """the program of the single-processor entry point behind ``case.call`` -- wf2wf: LOAD, op, STORE (in place for bl_subtract and the
    pole-zero filters); wf2scalars: LOAD, op, a STORE_SCALAR per output -- for dspeed_amd.chain.plan.  Only the shape matters to the
    planner's choice of a kernel: lengths, types, opcode, integer parameters; the scalar operands are constants here.  None: no processor"""
    from dspeed_amd import _lib as L
    from dspeed_amd.chain import Program, Scalar

    if case.call is None:
        return None
    n, ft, rows = case.n, case.ft, ROW_TYPES[case.tag]
    r, f, fall = trap_params(n)
    op, name = case.op, case.name
    col = lambda p, nm: Scalar.input(p.add_io(nm, L.IO_SCALAR_IN, ft))  # noqa: E731
    p = Program()
    scalars = {"fixed_time_pickoff": (L.OP_PICKOFF, 1), "time_point_thresh": (L.OP_TIME_POINT_THRESH, 1),
               "interpolated_time_point_thresh": (L.OP_INTERP_TIME_POINT_THRESH, 1), "min_max": (L.OP_MIN_MAX, 4),
               "mean_below_threshold": (L.OP_MEAN_BELOW, 1), "linear_slope_fit": (L.OP_LINEAR_SLOPE_FIT, 4), "trap_pickoff": (L.OP_TRAP_WINDOW_PICKOFF, 1)}
    if op in scalars:
        code, k = scalars[op]
        p.slots, p.n_sregs = [n], k
        io_in = p.add_io("wf", L.IO_WF_IN, rows, n)
        p.add_op(L.OP_LOAD, dst=0, io=io_in)
        ip, sp = (), ()
        if op == "fixed_time_pickoff":
            ip, sp = (ord(name[-1]),), (col(p, "t_in"),)
        elif op == "time_point_thresh":
            sp = (col(p, "thr"), col(p, "t_start"), Scalar.const(float(name[-1])))
        elif op == "interpolated_time_point_thresh":
            ip, sp = (ord(name[-1]),), (col(p, "thr"), col(p, "t_start"), Scalar.const(float(name[-3])))
        elif op == "mean_below_threshold":
            sp = (col(p, "thr"),)
        elif op == "trap_pickoff":
            ip, sp = (r, f), (col(p, "t_pk"),)
        p.add_op(code, dst=0, src=0, ip=ip, sp=sp)
        for j in range(k):
            p.add_op(L.OP_STORE_SCALAR, io=p.add_io(f"out{j}", L.IO_SCALAR_OUT, ft), ip=(j,))
        return p
    m = case.outs[0][1]
    if op == "min_max_norm":
        p.slots = [n]
        p.add_op(L.OP_LOAD, dst=0, io=p.add_io("wf", L.IO_WF_IN, rows, n))
        lo, hi = col(p, "a_lo"), col(p, "a_hi")
        p.add_op(L.OP_MIN_MAX_NORM, dst=0, src=0, sp=(lo, hi))
        p.add_op(L.OP_STORE, src=0, io=p.add_io("out", L.IO_WF_OUT, ft, n))
        return p
    if op == "convolve_wf":
        taps = int(name.split("-")[2][:-4])
        p.slots = [n, m]
        io_in = p.add_io("wf", L.IO_WF_IN, rows, n)
        io_k = p.add_io("taps", L.IO_TAPS, ft, taps)
        p.add_op(L.OP_LOAD, dst=0, io=io_in)
        p.add_op(L.OP_CONVOLVE, dst=1, src=0, io=io_k, ip=(ord(name.split("-")[1]), 0))
        p.add_op(L.OP_STORE, src=1, io=p.add_io("out", L.IO_WF_OUT, ft, m))
        return p
    if op == "moving_window_multi":
        num, typ = int(name.split("-")[1]), int(name[-1])
        p.slots = [n, n] + ([n] if num > 1 else [])
        p.add_op(L.OP_LOAD, dst=0, io=p.add_io("wf", L.IO_WF_IN, rows, n))
        p.add_op(L.OP_MOVING_WINDOW_MULTI, dst=1, src=0, ip=(typ, num, 2 if num > 1 else 0), sp=(Scalar.const(max(1, n // 10)),))
        p.add_op(L.OP_STORE, src=1, io=p.add_io("out", L.IO_WF_OUT, ft, n))
        return p
    wf = {"bl_subtract": (L.OP_BL_SUBTRACT, (), "bl"), "pole_zero": (L.OP_POLE_ZERO, (), "tau"),
          "double_pole_zero": (L.OP_DOUBLE_POLE_ZERO, (), "dpz"), "trap_filter": (L.OP_TRAP_FILTER, (r, f, 0), None),
          "trap_norm": (L.OP_TRAP_NORM, (r, f, 0), None), "asym_trap_filter": (L.OP_ASYM_TRAP, (r, f, fall), None),
          "windower": (L.OP_WINDOWER, (), "t0"), "avg_current": (L.OP_AVG_CURRENT, (), "L"), "upsampler": (L.OP_UPSAMPLER, (), "up"),
          "discrete_wavelet_transform": (L.OP_DWT_HAAR, None, None)}
    code, ip, operand = wf[op]
    in_place = op in ("bl_subtract", "pole_zero", "double_pole_zero") and m == n
    p.slots = [n] if in_place else [n, m]
    dst = 0 if in_place else 1
    p.add_op(L.OP_LOAD, dst=0, io=p.add_io("wf", L.IO_WF_IN, rows, n))
    if operand in ("bl", "t0"):
        sp = (col(p, operand),)
    elif operand == "tau":
        sp = (Scalar.const(max(1.5, n / 3.0)),)
    elif operand == "dpz":
        sp = (Scalar.const(max(2.0, n / 3.0)), Scalar.const(max(1.25, n / 40.0)), Scalar.const(0.02))
    elif operand == "L":
        sp = (Scalar.const(max(1, n // 10)),)
    elif operand == "up":
        sp = (Scalar.const(float(name.split("x")[1])),)
    else:
        sp = ()
    if op == "discrete_wavelet_transform":
        ip = (int(name[-2]), ord(name[-1]), 0)
    p.add_op(code, dst=dst, src=0, ip=ip, sp=sp)
    p.add_op(L.OP_STORE, src=dst, io=p.add_io("out", L.IO_WF_OUT, ft, m))
    return p


def route_a(case):
    """the kernel that form A's program plans onto (dspeed_amd.chain.plan: no device needed), or the error's type where the planner
    refuses it.  An op that is no processor (numpy.amax, a slice, where) stands alone in a recipe under the default routing instead"""
    from dspeed_amd.chain import plan
    from dspeed_amd.processing_chain import build_processing_chain

    try:
        program = processor_program(case)
        if program is None:
            register_taps_loader()
            names = [o[0] for o in case.outs]
            decl = [f"{k}({length}, '{'d' if case.tag == 'f64' else 'f'}')" if length else k for k, length in case.outs]
            chain, _, _ = build_processing_chain({"outputs": names, "processors": {", ".join(names): case._proc("waveform", decl)}},
                                                 {"waveform": case.rows, **case.cols})
            program = chain.program
        return plan(program, case.ft)["kernel"]
    except Exception as e:  # noqa: BLE001  (the table records what the planner says)
        return type(e).__name__
