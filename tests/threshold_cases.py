"""Cases of multi_time_point_thresh and time_over_threshold (dsp_thresh.hip): the rows, threshold lists and starting samples that
tools/gen_golden_thresholds.py feeds to the reference's bodies (tests/golden/thresholds.npz holds them with what the bodies returned), a
NumPy model of the kernel's formulation -- the thresholds ranked, then the two merged walks 64 samples a step with wrap-around reads --
that test_threshold_cases_cpu.py holds against the fixtures before anything runs on a GPU, and the model of m INDEPENDENT walks that the
same test shows to be wrong.  Nothing here needs a GPU or the reference.  Every row comes from a seed."""
import numpy as np

BOOK = "thresholds"
KERNEL = "multi_time_point_thresh"
LENGTHS = (2, 3, 63, 64, 65, 129, 1000, 1024, 8192)  # (1000, 129, 65, 63, 3, 2: no whole 16-byte vectors in one type or another)
MS = (1, 2, 7, 20, 64)
POLARITIES = (1.0, -1.0, 3.0, -2.0)
MODES = "iafbcrnl"
THRESH_MAX = 64
FAMILIES = ("ties", "walk", "pulse", "constant", "nan_last", "unanchored")
LISTS = ("spread", "above", "below", "dup", "inf", "nan", "blocked")
STARTS = ("mid", "half", "zero", "last", "neg", "n", "nan")
_ROW_TYPES = {"f32": np.float32, "f64": np.float64, "i16": np.int16, "u16": np.uint16}


class Group:
    """Rows of one length and type that go through one launch per (polarity, mode): ``w`` (R, n) in the rows' own type, ``thr`` (R, m) and
    ``ts`` (R,) in the loop's type -- every row its own (``shared`` false) or one list and one start for all --, ``tot_thr`` (R,) the
    thresholds of time_over_threshold, the rows' names (family:list:start) and the (polarity, mode) pairs the reference ran."""

    def __init__(self, name, tag, rows, w, thr, ts, tot_thr, names, combos, shared):
        self.name, self.tag, self.rows, self.w, self.thr, self.ts, self.tot_thr = name, tag, rows, w, thr, ts, tot_thr
        self.names, self.combos, self.shared = names, combos, shared
        self.loop = np.float32 if tag == "f32" else np.float64
        self.n, self.m = w.shape[1], thr.shape[1]


def key(pol, mode):
    return f"t_{'p' if pol > 0 else 'm'}{abs(int(pol))}_{mode}"


def _row(family, n, rng, integer):
    """(samples as float64, a sample in the middle of what happens in the row)"""
    i = np.arange(n, dtype=np.float64)
    mid = int(rng.integers(n // 4, max(n // 4 + 1, (3 * n) // 4)))
    if family == "ties" or (family == "nan_last" and integer):
        return rng.integers(-5, 6, n).astype(np.float64), mid
    if family == "nan_last":
        w = rng.integers(-5, 6, n).astype(np.float64)
        w[-1] = np.nan
        return w, mid
    if family == "walk":
        w = np.cumsum(rng.integers(-8, 9, n)) / (1.0 if integer else 4.0)
        return w, mid
    if family == "pulse":
        amp, c, width = rng.uniform(50, 200), n * rng.uniform(0.3, 0.7), max(1.0, n / 20)
        w = amp / (1 + np.exp(-(i - c) / width)) + amp / 50 * rng.standard_normal(n)
        if rng.random() < 0.5:
            w = -w
        return (np.rint(w) if integer else np.rint(w * 16) / 16), min(n - 1, int(c))
    if family == "constant":
        return np.full(n, 3.0), mid
    assert family == "unanchored" and n >= 4
    # at and behind the start the row stays at 3 or above, ahead of it at 2 or below, and falls from 1 to -4 just ahead of the start: with
    # polarity < 0 the lower walk's first pair is (ts - 2, ts - 1), which a threshold of 2 -- below w[ts], so the first of the lower group --
    # never crosses downwards there or later; thresholds of -1 and -3 are crossed in that pair, and a walk of their own would find them
    ts = int(rng.integers(2, n))
    w = np.concatenate([rng.integers(-5, 3, ts), rng.integers(3, 6, n - ts)]).astype(np.float64)
    w[ts - 2], w[ts - 1] = 1, -4
    return w, ts


def _list(kind, m, w, a, rng, integer):
    lo, hi = np.nanmin(w), np.nanmax(w)
    a = 0.0 if np.isnan(a) else a

    def spread(k):
        return rng.integers(int(lo) - 1, int(hi) + 2, k).astype(np.float64) if integer else np.rint(rng.uniform(lo - 1, hi + 1, k) * 8) / 8

    if kind == "blocked":
        t = np.concatenate([[2.0, -1.0, -3.0][:m], spread(m)[: max(0, m - 3)]])
    elif kind == "above":
        t = a + np.abs(spread(m) - a)
    elif kind == "below":
        t = a - np.abs(spread(m) - a) - 1
    elif kind == "dup":
        t = spread(max(1, m // 2))[rng.integers(0, max(1, m // 2), m)]
    else:
        t = spread(m)
        if kind == "inf":
            t[rng.integers(0, m)] = np.inf
            if m >= 2:
                t[rng.integers(0, m)] = -np.inf
        elif kind == "nan":
            t[rng.integers(0, m)] = np.nan
    return rng.permutation(t)


def _start(kind, n, mid):
    return {"mid": float(mid), "half": mid + 0.5, "zero": 0.0, "last": float(n - 1), "neg": -1.0, "n": float(n), "nan": np.nan}[kind]


def _group(name, tag, n, m, rows, shared, combos, rng):
    integer = tag in ("i16", "u16")
    loop = np.float32 if tag in ("f32", "i16", "u16") else np.float64
    offset = 100.0 if tag == "u16" else 0.0  # (unsigned rows: everything moves up)
    W, T, S, names = [], [], [], []
    shared_list = shared_start = None
    for r in range(rows):
        family = rng.choice(FAMILIES[:5], p=[0.35, 0.25, 0.3, 0.04, 0.06])
        if r < 2 and m >= 2 and n >= 4 and not shared:
            family = "unanchored"
        w, mid = _row(family, n, rng, integer)
        kind = "blocked" if family == "unanchored" else rng.choice(LISTS[:6], p=[0.5, 0.1, 0.1, 0.15, 0.1, 0.05])
        start = "mid" if family == "unanchored" else rng.choice(STARTS, p=[0.5, 0.17, 0.1, 0.1, 0.05, 0.04, 0.04])
        ts = _start(start, n, mid)
        if shared:  # one list and one start for every row: made for the first row
            if shared_list is None:
                kind, start = "spread", "mid"
                ts = _start(start, n, mid)
                shared_list, shared_start = _list(kind, m, np.array([-5.0, 5.0]), 0.0, rng, True), ts
            thr, ts, kind, start = shared_list, shared_start, "shared", "shared"
        else:
            at = int(ts) if 0 <= ts < n else mid
            thr = _list(kind, m, w, w[at], rng, integer or family in ("ties", "nan_last", "constant", "unanchored"))
        W.append(w + offset)
        T.append(thr + offset)
        S.append(ts)
        names.append(f"{family}:{kind}:{start}")
    w = np.array(W)
    w = w.astype(_ROW_TYPES[tag]) if integer else w.astype(loop)
    tot = np.array([np.nan if rng.random() < 0.08 else (rng.integers(-3, 4) + offset) for _ in range(rows)])
    return Group(name, "f32" if loop == np.float32 else "f64", tag, w, np.array(T).astype(loop), np.array(S).astype(loop), tot.astype(loop), names, combos,
                 shared)


def groups():
    """every group of the book, in a fixed order"""
    rng = np.random.default_rng(20261019)
    out, k, seen = [], 0, [0, 0]
    for li, n in enumerate(LENGTHS):
        tags = ("f32", "f64") + (("i16", "u16") if n in (65, 1000, 1024) else ())
        for ti, tag in enumerate(tags):
            ms = MS if (tag == "f32" and n in (65, 1000)) else (MS[(li + ti) % len(MS)],)
            for m in ms:
                q = seen[tag == "f64"]  # (the polarities rotate through the modes within each loop)
                seen[tag == "f64"] += 1
                combos = [(POLARITIES[(j + q) % 4], MODES[j]) for j in range(8)]
                out.append(_group(f"{tag}_n{n}_m{m}", tag, n, m, 8 if n == 8192 else (13 if n >= 1000 else 22), k % 3 == 2, combos, rng))
                k += 1
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# the kernel's formulation
# ------------------------------------------------------------------------------------------------------------------------------------
def _time(mode, pol, i, wi, wn, thr, T):
    """the time of a crossing between w[i] = wi and w[i + pol] = wn, in the loop's type"""
    with np.errstate(all="ignore"):
        if mode == "i":
            return T(i)
        if mode in "af":
            return T(i if pol < 0 else i + 1)
        if mode in "bc":
            return T(i if pol > 0 else i - 1)
        if mode == "r":
            return T(i if T(thr - wi) < T(wn - thr) else i + pol)
        if mode == "n":
            return T(i + 0.5 * pol)
        assert mode == "l"
        return T(T(i) + T(T(thr - wi) / T(wn - wi)))


def _nan_row(w, thr, ts):
    return bool(np.isnan(w).any() or np.isnan(thr).any() or np.isnan(ts) or ts < 0 or ts >= len(w))


def model(w, thr, ts, polarity, mode, T, lanes=64):
    """dsp_thresh_kernel on one row: ``w`` and ``thr`` in the loop's type T.  Rank, permute, two walks of ``lanes`` samples a step."""
    w, thr = np.asarray(w, dtype=T), np.asarray(thr, dtype=T)
    n, m = len(w), len(thr)
    out = np.full(m, np.nan, dtype=T)
    if m == 0 or _nan_row(w, thr, ts):
        return out
    ts, pol = int(ts), (1 if polarity > 0 else -1)
    # rank: thresholds below, or equal with a lower index; the permutation puts value and index at lane `rank`
    idx = np.arange(m)
    rank = np.array([int(np.sum((thr < thr[j]) | ((thr == thr[j]) & (idx < j)))) for j in range(m)])
    sorted_thr, index = np.empty(m, dtype=T), np.empty(m, dtype=np.int64)
    sorted_thr[rank], index[rank] = thr, idx
    i_start = int(np.sum(thr < w[ts]))
    res = np.full(m, np.nan, dtype=T)
    lane = np.arange(lanes)

    def at(j):  # (negative indices wrap: j >= -2, n >= 2)
        return w[np.where(j < 0, j + n, j)]

    def walk(i0, step, lo, hi, tp, tstep):
        base = i0
        while 0 <= tp < m and lo <= base <= hi:
            cur = sorted_thr[tp]
            i = base + step * lane
            live = (i >= lo) & (i <= hi)
            ic = np.where(live, i, lo)
            wi, wn = at(ic), at(ic + pol)
            hits = live & (wi <= cur) & (cur < wn)
            if hits.any():
                first = int(np.argmax(hits))
                res[tp] = _time(mode, pol, int(i[first]), wi[first], wn[first], cur, T)
                tp += tstep
                base += step * first
            else:
                base += step * lanes

    if pol > 0:
        walk(ts, 1, ts, n - 2, i_start, 1)
        walk(ts - 1, -1, 0, ts - 1, i_start - 1, -1)
    else:
        walk(ts, -1, 0, ts, i_start, 1)
        walk(ts - 1, 1, ts - 1, n - 2, i_start - 1, -1)
    out[index] = res
    return out


def independent(w, thr, ts, polarity, mode, T):
    """The WRONG model: every threshold on a walk of its own -- the first i from the start at which the test holds.  It differs from the
    reference where the thresholds' chain matters (a threshold that is never crossed blocks those sorted behind it)."""
    w, thr = np.asarray(w, dtype=T), np.asarray(thr, dtype=T)
    n, m = len(w), len(thr)
    out = np.full(m, np.nan, dtype=T)
    if m == 0 or _nan_row(w, thr, ts):
        return out
    ts, pol = int(ts), (1 if polarity > 0 else -1)
    upper = range(ts, n - 1 if pol > 0 else -1, pol)
    lower = range(ts - 1, n - 1 if pol < 0 else -1, -pol)
    for j in range(m):
        for i in (upper if thr[j] >= w[ts] else lower):
            if w[i] <= thr[j] < w[i + pol]:
                out[j] = _time(mode, pol, i, w[i], w[i + pol], thr[j], T)
                break
    return out


def model_time_over_threshold(w, thr, T):
    w = np.asarray(w, dtype=T)
    if np.isnan(w).any() or np.isnan(thr):
        return T(np.nan)
    return T(np.count_nonzero(w > T(thr)))


# the rows of the recipe test (test_gpu_thresholds.py): 24 rows of 1000 uint16 samples, a rising pulse on a pedestal
RECIPE_ROWS, RECIPE_N = 24, 1000


def recipe_rows():
    rng = np.random.default_rng(909)
    i = np.arange(RECIPE_N, dtype=np.float64)[None, :]
    amp, c = rng.uniform(500, 3000, (RECIPE_ROWS, 1)), rng.uniform(300, 600, (RECIPE_ROWS, 1))
    w = 1000 + amp / (1 + np.exp(-(i - c) / 12.0)) + 3 * rng.standard_normal((RECIPE_ROWS, RECIPE_N))
    return np.rint(w).astype(np.uint16)


# ------------------------------------------------------------------------------------------------------------------------------------
# programs (test_threshold_plan_cpu.py, test_gpu_thresholds.py)
# ------------------------------------------------------------------------------------------------------------------------------------
def multi_program(n, m, rows_dtype=np.float32, loop=np.float32, lists=False, t_start=0.0, polarity=1.0, mode="l", offset=0, row_stride=None):
    """LOAD, [LOAD of a list per row,] MULTI_TIME_POINT_THRESH, STORE; bindings wf, thr (a DSP_IO_TAPS vector, or rows with ``lists``),
    t_start (a column when ``t_start`` is "column"), t_out"""
    from dspeed_amd import _lib
    from dspeed_amd.chain import Program, Scalar

    p = Program()
    p.slots = [n, m] + ([m] if lists else [])
    p.add_op(_lib.OP_LOAD, dst=0, io=p.add_io("wf", _lib.IO_WF_IN, rows_dtype, n, offset, row_stride))
    if lists:
        p.add_op(_lib.OP_LOAD, dst=2, io=p.add_io("thr", _lib.IO_WF_IN, loop, m))
        io, slot = 0, 2
    else:
        io, slot = p.add_io("thr", _lib.IO_TAPS, loop, m), -1
    ts = Scalar.input(p.add_io("t_start", _lib.IO_SCALAR_IN, loop)) if isinstance(t_start, str) else Scalar.const(t_start)
    pol = Scalar.input(p.add_io("polarity", _lib.IO_SCALAR_IN, loop)) if isinstance(polarity, str) else Scalar.const(polarity)
    p.add_op(_lib.OP_MULTI_TIME_POINT_THRESH, dst=1, src=0, io=io, ip=(ord(mode), slot), sp=(ts, pol))
    p.add_op(_lib.OP_STORE, src=1, io=p.add_io("t_out", _lib.IO_WF_OUT, loop, m))
    return p


def over_program(n, rows_dtype=np.float32, loop=np.float32, threshold=0.0):
    """LOAD, TIME_OVER_THRESHOLD, STORE_SCALAR; bindings wf, threshold (a column when ``threshold`` is "column"), count"""
    from dspeed_amd import _lib
    from dspeed_amd.chain import Program, Scalar

    p = Program()
    p.slots, p.n_sregs = [n], 1
    p.add_op(_lib.OP_LOAD, dst=0, io=p.add_io("wf", _lib.IO_WF_IN, rows_dtype, n))
    thr = Scalar.input(p.add_io("threshold", _lib.IO_SCALAR_IN, loop)) if isinstance(threshold, str) else Scalar.const(threshold)
    p.add_op(_lib.OP_TIME_OVER_THRESHOLD, dst=0, src=0, sp=(thr,))
    p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io("count", _lib.IO_SCALAR_OUT, loop), ip=(0,))
    return p


def over_half_recipe():
    """time_over_threshold of the INPUT rows above half the maximum of the baseline-subtracted waveform: the threshold is read off a waveform
    the program computes itself, so it is written to memory ahead of the stage"""
    M = "dspeed.processors"
    return {
        "wf_blsub": {"function": "bl_subtract", "module": M, "args": ["waveform", "bl", "wf_blsub"]},
        "tp_min, tp_max, wf_min, wf_max": {"function": "min_max", "module": M, "args": ["wf_blsub", "tp_min", "tp_max", "wf_min", "wf_max"]},
        "n_over": {"function": "time_over_threshold", "module": M, "args": ["waveform", "0.5*wf_max", "n_over"]},
    }


def rise_time_recipe(source="waveform", unit=None):
    """bl_subtract -> min_max -> min_max_norm -> multi_time_point_thresh at 10 / 50 / 90 % from the maximum backwards, and the time over
    half the maximum: the processors of a recipe as the reference writes them"""
    M = "dspeed.processors"
    tps = {"function": "multi_time_point_thresh", "module": f"{M}.time_point_thresh", "args": ["wf_norm", "[0.1, 0.5, 0.9]", "t_hi", 1, "'l'", "tps(3)"]}
    t_sat = {"function": "time_over_threshold", "module": f"{M}.time_over_threshold", "args": ["wf_blsub", "0.5*wf_max", "t_sat"]}
    if unit:
        tps["unit"], t_sat["unit"] = unit, unit
    return {
        "wf_blsub": {"function": "bl_subtract", "module": M, "args": [source, "bl", "wf_blsub"]},
        "tp_min, tp_max, wf_min, wf_max": {"function": "min_max", "module": M, "args": ["wf_blsub", "tp_min", "tp_max", "wf_min", "wf_max"]},
        "wf_norm": {"function": "min_max_norm", "module": M, "args": ["wf_blsub", "wf_min", "wf_max", "wf_norm"]},
        "t_lo, t_hi, a_lo, a_hi": {"function": "min_max", "module": M, "args": ["wf_norm", "t_lo", "t_hi", "a_lo", "a_hi"]},
        "tps": tps, "t_sat": t_sat,
    }
