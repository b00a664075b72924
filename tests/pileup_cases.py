"""The case book of the pile-up finder -- rc_cr2 (reference processors/rc_cr2.py:12-94) and bi_level_zero_crossing_time_points
(processors/time_point_thresh.py:404-532) -- and a NumPy emulation of both bodies, both loops: the yardstick of tests/test_gpu_pileup.py,
itself held to the reference bodies' recorded results by tests/test_pileup_cases_cpu.py (tests/golden/pileup.npz, written by
tools/gen_golden_pileup.py).

Every row is made of integer draws and float64 additions and multiplications only, so the book is the same on every machine.

The filter's pole a = exp(-1 / t_tau) has three sources here, because the last bit of an exponential is the library's that computes it:
``a=`` a given value (the fixture records the one the reference run used), ``exp="numpy"`` NumPy's (what the reference body calls under
CPython) and ``exp="libm"`` the C library's (what numba compiles the body to, and what the planner calls on the host).  Its cube has two
rules: ``cube="pow"`` is CPython's ``a**2`` / ``a**3``, ``cube="product"`` numba's a * a / a * (a * a), which the device is held to."""
import math

import numpy as np

from dspeed_amd import _lib

BOOK = "pileup"
KERNEL = "dsp_pileup_kernel"
LOOPS = {"f32": np.float32, "f64": np.float64}
LENGTHS = (4, 5, 63, 64, 65, 127, 128, 129, 257)  # the filter's minimum, and both sides of every edge of the 64-sample tile
TAUS = (20, 100, 500)  # at 20 and 100 pow(a, 3) != a * (a * a), at 500 they are equal
MS = (1, 5, 30)
ROW_COUNTS = (1, 63, 64, 65, 130)  # dead lanes and partial wavefronts
NAN = float("nan")


# ---------------------------------------------------------------------------------------------------------------- the filter
def pole(tau, T, exp="numpy"):
    """a = exp(-1 / t_tau) in float64 whatever the loop, t_tau carrying the loop type's value (numba's typing of int64 / float32)"""
    t = float(T(tau))
    if t != t:
        return NAN
    with np.errstate(all="ignore"):
        return float(np.exp(np.float64(-1.0) / np.float64(t))) if exp == "numpy" else (math.exp(-1.0 / t) if t != 0 else 0.0)


def coefficients(a, cube):
    """3a, 3 a^2, a^3 as float64 (rc_cr2.py:68-71)"""
    a = np.float64(a)
    with np.errstate(all="ignore"):
        if cube == "pow":
            return 3 * a, 3 * a**2, a**3
        assert cube == "product"
        return 3 * a, 3 * (a * a), a * (a * a)


def emulate_rc_cr2(rows, tau, T, cube="product", exp="numpy", a=None, state=False):
    """(w_out, fatal): the body's sum in the written order on a float64 state, one rounding at the store; ``fatal`` marks the rows on which
    the reference raises DSPFatal("RC-CR^2 filter produced nans in output.") -- their output is what the body had written by then.
    ``state``: the float64 values before the store instead (what a fused walk must NOT read)."""
    x = np.atleast_2d(np.asarray(rows)).astype(T).astype(np.float64)
    n_rows, n = x.shape
    assert n > 3
    a = pole(tau, T, exp) if a is None else a
    c1, c2, c3 = coefficients(a, cube)
    res = x.copy()
    w0, w1, w2 = x[:, 0].copy(), x[:, 1].copy(), x[:, 2].copy()
    with np.errstate(all="ignore"):
        for i in range(3, n):
            s = c1 * w2
            s = s - c2 * w1
            s = s + c3 * w0
            s = s + x[:, i]
            s = s + -2.0 * x[:, i - 1]
            s = s + x[:, i - 2]
            res[:, i] = s
            w0, w1, w2 = w1, w2, s
        out = res.astype(T)
    nan_row = np.isnan(x).any(axis=1) | bool(np.isnan(T(tau)))
    out[nan_row] = np.nan
    res[nan_row] = np.nan
    fatal = ~nan_row & np.isnan(out).any(axis=1)
    return (res if state else out), fatal


def _draws(seed, n, lo, hi):
    return np.random.default_rng(seed).integers(lo, hi, n).astype(np.float64)


def _decay(n, amplitude, keep):
    """amplitude * keep^k by repeated multiplication"""
    out = np.empty(n)
    v = float(amplitude)
    for k in range(n):
        out[k] = v
        v *= keep
    return out


FILTER_FAMILIES = ("step", "two-steps", "noise", "integer", "alternating", "ramp", "tiny", "nan-first", "nan-middle", "nan-last", "inf", "minus-inf-last")
FILTER_FATAL = ("inf",)  # (an infinity in the last sample makes no NaN: nothing reads it back)


def filter_rows(loop, n):
    """the rows rc_cr2 is run on, a family per row (FILTER_FAMILIES), in the loop's type"""
    rows = np.zeros((len(FILTER_FAMILIES), n))
    f = FILTER_FAMILIES.index
    lead = min(5, n // 4)
    rows[f("step"), lead:] = _decay(n - lead, 1750.0, 0.99996)
    rows[f("two-steps")] = rows[f("step")]
    rows[f("two-steps"), n // 2:] += _decay(n - n // 2, 900.0, 0.99996)
    rows[f("noise")] = _draws(11 + n, n, -4000, 4000) / 8
    rows[f("integer")] = 1000 + _draws(12 + n, n, -40, 40)  # (what a digitiser writes: also the uint16 / int16 rows of the C entries' test)
    rows[f("integer"), n // 3:] += 300
    rows[f("alternating")] = np.where(np.arange(n) % 2 == 0, 10.0, -10.0)
    rows[f("ramp")] = np.arange(n) * 3.25 - 7
    rows[f("tiny")] = _draws(13 + n, n, -9, 9) * 2.0**-120
    for name, at in (("nan-first", 0), ("nan-middle", n // 2), ("nan-last", n - 1)):
        rows[f(name)] = rows[f("noise")]
        rows[f(name), at] = np.nan
    rows[f("inf")] = rows[f("noise")]
    rows[f("inf"), 0] = np.inf
    rows[f("minus-inf-last")] = rows[f("noise")]
    rows[f("minus-inf-last"), n - 1] = -np.inf
    return rows.astype(LOOPS[loop])


def filter_cases(loop):
    """(key, n, tau) of the filter's part of the book; a NaN t_tau once per length"""
    for n in LENGTHS:
        for tau in TAUS:
            yield f"rc_cr2_{loop}_n{n}_tau{tau}", n, tau
        yield f"rc_cr2_{loop}_n{n}_taunan", n, NAN


# ---------------------------------------------------------------------------------------------------------------- the walk
def emulate_walk(rows, pos, neg, gate, t_start, m, T):
    """(n_crossings uint32, polarity, times): the reference's state machine, its two state variables holding the sample index and tested
    for truth.  The candidates start at 0 (the reference leaves them unbound until a zero crossing is seen; no row of the book reads one
    before: tools/gen_golden_pileup.py would fail there).  A NaN row or operand, or a gate that is not finite: NaN lists, count 0."""
    w_all = np.atleast_2d(np.asarray(rows)).astype(T)
    n_rows, n = w_all.shape
    col = lambda v: np.broadcast_to(np.asarray(v, dtype=T), (n_rows,))  # noqa: E731
    pos, neg, gate, t_start = col(pos), col(neg), col(gate), col(t_start)
    count = np.zeros(n_rows, np.uint32)
    polarity, times = np.full((n_rows, m), np.nan, T), np.full((n_rows, m), np.nan, T)
    for r in range(n_rows):
        w, p, q, g, t = w_all[r].tolist(), float(pos[r]), float(neg[r]), float(gate[r]), float(t_start[r])
        if np.isnan(w_all[r]).any() or p != p or q != q or t != t or not math.isfinite(g):
            continue
        assert math.floor(t) == t and 0 <= int(t) < n, "the book holds no start that raises"
        g = int(g)
        above = below = 0
        crossed = False
        pos_cand = neg_cand = 0
        k = 0
        for i in range(int(t), n - 1):
            wi, wn = w[i], w[i + 1]
            if below and wi <= 0 < wn:
                crossed, neg_cand = True, i
            if wi <= p < wn:
                if crossed and below:
                    if i - below < g:
                        if k < m:
                            times[r, k], polarity[r, k] = neg_cand, 0
                        k += 1
                    else:
                        above = i
                    below, crossed = 0, False
                else:
                    above = i
            if above and wi >= 0 > wn:
                crossed, pos_cand = True, i
            if wi >= q > wn:
                if crossed and above:
                    if i - above < g:
                        if k < m:
                            times[r, k], polarity[r, k] = pos_cand, 1
                        k += 1
                    else:
                        below = i
                    above, crossed = 0, False
                else:
                    below = i
        count[r] = k
    return count, polarity, times


SAMPLE0 = [0, 10, -10, 10, -10, 10, -10, 0, 0, 0]  # thresholds +-1, gate 10, start 0: 2 crossings of polarity 0 at [2, 4] -- the first threshold
SAMPLE0_TWIN = [0] + SAMPLE0                       # crossing, at sample 0, counts as not set; behind one more 0: 3 of polarity 1 at [2, 4, 6]


def _fit(values, n):
    out = np.zeros(n)
    k = min(n, len(values))
    out[:k] = values[:k]
    return out


def pulses(n, a=0.9375):
    """two rc_cr2-shaped pulses: two steps through the filter with an exactly representable pole (the reference test's construction,
    shortened), scaled to a peak of about 1000"""
    if n < 8:
        return _fit([0, 400, 900, -300, -500], n)
    step = np.zeros(n + 5)
    step[5:] = _decay(n, 1750.0, 0.99996)
    step[5 + n // 2:] += _decay(n - n // 2, 1200.0, 0.99996)
    out, _ = emulate_rc_cr2(step, 0.0, np.float64, a=a)
    out = out[0, 5:]
    return out * (1000.0 / np.abs(out).max())


def walk_case(loop, n, m):
    """One case of the walk: rows of n samples with an operand set per row (name, row, pos, neg, gate, t_start)."""
    T = LOOPS[loop]
    slow = np.tile([0.0, 5, 10, 5, 0, -5, -10, -5], n // 8 + 1)[:n]  # i - state is 4 from a threshold crossing to the next of the other sign
    alternating = np.concatenate([[0.0], np.where(np.arange(n - 1) % 2 == 0, 10.0, -10.0)])
    noise = _draws(21 + n, n, -40, 40) / 4
    on_thr = np.tile([0.0, 1, 2, 1, 0, -0.0, -1, -2, -1, 0.0, 0.5, 2, -0.0, -2], n // 14 + 1)[:n]  # samples on +-1, on 0.0 and on -0.0
    p2 = pulses(n)
    nan_row = noise.copy()
    nan_row[n // 2] = np.nan
    inf_row = slow.copy()
    inf_row[min(2, n - 1)] = np.inf
    inf_row[min(6, n - 1)] = -np.inf
    out = [
        ("pulses", p2, 200, -200, 1000, 0), ("pulses-tight-gate", p2, 200, -200, 3, 0), ("pulses-late", p2, 200, -200, 1000, n // 2),
        ("alternating", alternating, 1, -1, 10, 0), ("alternating-overflow", alternating, 5, -5, 2, 0),
        ("sample0", _fit(SAMPLE0, n), 1, -1, 10, 0), ("sample0-twin", _fit(SAMPLE0_TWIN, n), 1, -1, 10, 0),
        ("on-threshold", on_thr, 1, -1, 10, 0), ("on-threshold-zero", on_thr, 0, -0.0, 10, 0), ("on-threshold-late", on_thr, 1, -1, 100, min(3, n - 1)),
        ("nan", nan_row, 3, -3, 10, 0), ("inf", inf_row, 7, -7, 10, 0), ("inf-threshold", slow, np.inf, -np.inf, 10, 0),
        ("mono-up", np.arange(n) * 2.5 - 3, 1, -1, 10, 0), ("mono-down", 3 - np.arange(n) * 2.5, 1, -1, 10, 0), ("zeros", np.zeros(n), 1, -1, 10, 0),
        ("nan-pos", slow, NAN, -7, 10, 0), ("nan-neg", slow, 7, NAN, 10, 0), ("nan-start", slow, 7, -7, 10, NAN), ("nan-start-nan-row", nan_row, 7, -7, 10, NAN),
    ]
    # the gate: i - state equal to it (not counted), one less (counted), 0, negative, fractional (int() cuts towards zero), beyond every row
    out += [(f"gate{g}", slow, 7, -7, g, 0) for g in (0, 1, 3, 4, 5, 8, -1, 4.5, 4.999, 5.5, -0.5, 3.0e9, -3.0e9)]
    out += [(f"start{t}", noise, 3, -3, 6, t) for t in sorted({0, 1, n // 2, n - 2, n - 1})]  # (n - 1: the loop is empty)
    out += [(f"start{t}-slow", slow, 7, -7, 5, t) for t in sorted({1, 2, 3, n // 2})]
    names = [o[0] for o in out]
    rows = np.stack([np.asarray(o[1], dtype=np.float64) for o in out]).astype(T)
    pos, neg, gate, ts = (np.array([o[k] for o in out], dtype=T) for k in (2, 3, 4, 5))
    return dict(key=f"walk_{loop}_n{n}_m{m}", n=n, m=m, names=names, rows=rows, pos=pos, neg=neg, gate=gate, t_start=ts)


def walk_cases(loop):
    for n in LENGTHS:
        for m in MS:
            yield walk_case(loop, n, m)


FUSED = [(n, tau, m) for n in (65, 129, 257) for tau in TAUS for m in (5,)]


def fused_case(loop, n, tau, m):
    """rc_cr2 of the filter's rows, then the walk of the filtered rows with thresholds at a tenth of each family's usual size"""
    rows = filter_rows(loop, n)
    fine = [k for k, f in enumerate(FILTER_FAMILIES) if f != "inf"]  # (the filter raises there)
    T = LOOPS[loop]
    return dict(key=f"fused_{loop}_n{n}_tau{tau}_m{m}", n=n, tau=tau, m=m, rows=rows[fine], names=[FILTER_FAMILIES[k] for k in fine],
                pos=T(40), neg=T(-40), gate=T(3 * tau), t_start=T(0))


def tile_rows(a, count):
    """``count`` rows (or values) that repeat those of ``a`` in turn"""
    a = np.asarray(a)
    return a[np.arange(count) % len(a)]


# ---------------------------------------------------------------------------------------------------------------- the rounding case
def rounding_case():
    """A float32-loop row on which the float64 state of the filter and its float32 rounding fall on opposite sides of a threshold: the
    positive threshold IS the stored value of a sample k that was rounded down, on a rising edge -- "threshold < stored" is false,
    "threshold < state" true -- so a walk of the state sees the crossing one sample earlier than a walk of the stored row, and the gate is
    the distance at which that sample decides whether the crossing counts.  (rows, tau, pos, neg, gate, k), the first such sample of the
    row on which the two walks give different results."""
    n, tau = 129, 20
    rows = filter_rows("f32", n)[[FILTER_FAMILIES.index("noise")]]
    stored, _ = emulate_rc_cr2(rows, tau, np.float32, exp="libm")
    state, _ = emulate_rc_cr2(rows, tau, np.float32, exp="libm", state=True)
    neg = np.float32(-100)
    for k in range(4, n):
        if not (state[0, k] > stored[0, k] > 0 and stored[0, k - 1] < stored[0, k]):
            continue
        pos = np.float32(stored[0, k])
        for gate in range(1, 48):
            of_stored = emulate_walk(stored, pos, neg, gate, 0, 5, np.float32)
            of_state = emulate_walk(state, pos, neg, gate, 0, 5, np.float64)
            if not np.array_equal(of_stored[0], of_state[0]):
                return rows, tau, pos, neg, np.float32(gate), k
    raise AssertionError("no sample of the row is rounded down on a rising edge where it decides a crossing")


# ---------------------------------------------------------------------------------------------------------------- programs
def program(n, rows=np.float32, loop=np.float32, filter=True, walk=False, m=5, store_row=True, tau=20.0, offset=0, row_stride=None, out_stride=None,
            out_len=None, list_lens=None, columns=(), list_stride=None, operands=(1.0, -1.0, 10.0, 0.0), subtract=None):
    """LOAD, [BL_SUBTRACT,] [RC_CR2,] [BI_LEVEL_ZERO_CROSSING,] [STORE of the filtered row,] [STORE, STORE, STORE_SCALAR]; ``columns``: the
    walk's operands that are per-event columns (indices 0 .. 3 of pos, neg, gate, t_start); ``subtract``: a baseline, or "column" for one per event"""
    from dspeed_amd.chain import Program, Scalar

    p = Program()
    s_in = p.add_slot(n)
    p.add_op(_lib.OP_LOAD, dst=s_in, io=p.add_io("w", _lib.IO_WF_IN, rows, n, offset, row_stride))
    src = s_in
    if subtract is not None:
        p.add_op(_lib.OP_BL_SUBTRACT, dst=s_in, src=s_in, sp=(Scalar.input(p.add_io("bl", _lib.IO_SCALAR_IN, loop)) if subtract == "column" else Scalar.const(subtract),))
    if filter:
        s_out = p.add_slot(n if out_len is None else out_len)
        tau_arg = Scalar.input(p.add_io("tau", _lib.IO_SCALAR_IN, loop)) if tau == "column" else Scalar.const(tau)
        p.add_op(_lib.OP_RC_CR2, dst=s_out, src=s_in, sp=(tau_arg,))
        src = s_out
    if walk:
        lens = (m, m) if list_lens is None else list_lens
        s_pol, s_time = p.add_slot(lens[0]), p.add_slot(lens[1])
        reg = p.add_sregs(1)
        names = ("pos", "neg", "gate", "t_start")
        sp = tuple(Scalar.input(p.add_io(names[k], _lib.IO_SCALAR_IN, loop)) if k in columns else Scalar.const(operands[k]) for k in range(4))
        p.add_op(_lib.OP_BI_LEVEL_ZERO_CROSSING, dst=s_pol, src=src, ip=(s_time, reg), sp=sp)
    if filter and store_row:
        p.add_op(_lib.OP_STORE, src=s_out, io=p.add_io("out", _lib.IO_WF_OUT, loop, p.slots[s_out], 0, out_stride))
    if walk:
        p.add_op(_lib.OP_STORE, src=s_pol, io=p.add_io("polarity", _lib.IO_WF_OUT, loop, lens[0], 0, list_stride))
        p.add_op(_lib.OP_STORE, src=s_time, io=p.add_io("times", _lib.IO_WF_OUT, loop, lens[1], 0, list_stride))
        p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io("count", _lib.IO_SCALAR_OUT, np.uint32), ip=(reg,))
    return p
