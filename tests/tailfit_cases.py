"""The case book of the decay-tail fitter -- log_check (reference processors/log_check.py:11-48), the gufunc poly_fit(length, deg) returns,
poly_diff and poly_exp_rms (processors/poly_fit.py:12-141) -- and a NumPy emulation of the four bodies, both loops: the yardstick of
tests/test_gpu_tailfit.py, itself held to the reference bodies' recorded results by tests/test_tailfit_cases_cpu.py
(tests/golden/tailfit.npz, written by tools/gen_golden_tailfit.py).

Every row is made of integer draws and float64 additions and multiplications only, so the book is the same on every machine.

THE TYPING TABLE.  Where numba and CPython type the bodies differently, numba's typing is the rule (w, p: the loop's type T; i, j: int64):
    i**j                    int64, exact (the planner refuses what would wrap); float64(i**j): one conversion, never a running product
    w[i] * (i**j)           float64 * float64 (float32 * int64 is float64 under numba; CPython with NumPy 2 would keep float32)
    arr[j] += ...           float64, ascending i
    inv @ arr               float64, here: acc = 0.0, acc = acc + inv[k][j] * arr[j] for ascending j; one rounding into T
    p[j] * i**j             float64 * float64; temp += ...: float64, ascending j, from 0.0
    w[i] - temp, - exp(temp)   float64; exp: the float64 exponential
    mean += r / (i + 1)     T(float64(mean) + r / float64(i + 1)): the array's in-place addition takes the float64 loop and casts back
    rms += r * r            T(float64(rms) + r * r)                (r ** 2 is r * r)
    rms /= n - 1            T(float64(rms) / float64(n - 1)); n = 1 divides by zero as IEEE does
    sqrt(rms)               in T
    log(w)                  in T
No operation is fused.  A row with a NaN: log_check and poly_fit give NaNs (poly_fit's is the product's rule: the reference leaves the
output untouched), the residuals NaN, NaN; so do NaN coefficients."""
import numpy as np

from dspeed_amd import _lib

BOOK = "tailfit"
KERNEL = "dsp_tailfit_kernel"
LOOPS = {"f32": np.float32, "f64": np.float64}
LENGTHS = (1, 2, 3, 63, 64, 65, 129)  # both sides of every edge of the 64-sample tile, and the shortest rows
ROW_COUNTS = (1, 63, 64, 65, 130)  # dead lanes and partial wavefronts
MS = (1, 2, 4, 8)
POLY_MAX = 8
NAN = float("nan")
HI = np.longdouble  # "one precision up" for both loops
U64 = 2.0**-53


def unit(T):
    return float(np.finfo(T).eps) / 2


def same(a, b):
    """bit for bit, a NaN being a NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a) & ~np.isnan(a), np.signbit(b) & ~np.isnan(b))


# ---------------------------------------------------------------------------------------------------------------- the emulation
def inverse(length, deg):
    """poly_fit.py:50-61 as written: float64 power sums over range(length), np.linalg.inv (a singular matrix, length <= deg, raises there)"""
    vals_array = np.zeros(2 * deg + 1, dtype="float64")
    for i in range(length):
        for j in range(2 * deg + 1):
            vals_array[j] += i**j
    mat = np.zeros((deg + 1, deg + 1), dtype="float")
    for i in range(deg + 1):
        mat[i, :] = vals_array[i: deg + 1 + i]
    return np.linalg.inv(mat)


def emulate_log_check(rows, T):
    x = np.atleast_2d(np.asarray(rows)).astype(T)
    with np.errstate(all="ignore"):
        out = np.log(x)
    bad = np.isnan(x).any(axis=1) | (x <= 0).any(axis=1)
    out[bad] = np.nan
    return out


def emulate_poly_fit(rows, inv, T):
    """the moments in float64 for ascending i, the product for ascending j, one rounding"""
    x = np.atleast_2d(np.asarray(rows)).astype(T).astype(np.float64)
    inv = np.asarray(inv, dtype=np.float64)
    m, (n_rows, n) = len(inv), x.shape
    arr = np.zeros((n_rows, m))
    with np.errstate(all="ignore"):
        for i in range(n):
            for j in range(m):
                arr[:, j] = arr[:, j] + x[:, i] * float(i**j)
        out = np.empty((n_rows, m))
        for k in range(m):
            acc = np.zeros(n_rows)
            for j in range(m):
                acc = acc + inv[k, j] * arr[:, j]
            out[:, k] = acc
        out = out.astype(T)
    out[np.isnan(x).any(axis=1)] = np.nan
    return out


def emulate_residual(rows, pars, T, exp_rms):
    """(mean, rms) of poly_diff (``exp_rms`` false) or poly_exp_rms: both sums round to T after every sample"""
    x = np.atleast_2d(np.asarray(rows)).astype(T)
    n_rows, n = x.shape
    p = np.broadcast_to(np.atleast_2d(np.asarray(pars)).astype(T), (n_rows, np.shape(pars)[-1])).astype(np.float64)
    m = p.shape[1]
    xd = x.astype(np.float64)
    mean, rms = np.zeros(n_rows, T), np.zeros(n_rows, T)
    with np.errstate(all="ignore"):
        for i in range(n):
            temp = np.zeros(n_rows)
            for j in range(m):
                temp = temp + p[:, j] * float(i**j)
            r = xd[:, i] - (np.exp(temp) if exp_rms else temp)
            mean = (mean.astype(np.float64) + r / float(i + 1)).astype(T)
            rms = (rms.astype(np.float64) + r * r).astype(T)
        rms = np.sqrt((rms.astype(np.float64) / np.float64(n - 1)).astype(T))
    bad = np.isnan(x).any(axis=1) | np.isnan(p).any(axis=1)
    mean[bad] = np.nan
    rms[bad] = np.nan
    return mean, rms


# ---------------------------------------------------------------------------------------------------------------- the bounds
def _ulp(v, T):
    with np.errstate(all="ignore"):
        return np.spacing(np.abs(np.asarray(v).astype(T))).astype(np.float64)


def log_bound(rows, T):
    """(exact, bound) of log_check's values.  Both logarithms involved -- NumPy's in T, the yardstick's, and the device's -- are documented
    to one ulp of T, so each lies within ulp_T(exact) of the exact value; ``exact`` is evaluated one precision up, whose own error (four of
    its units) is added."""
    x = np.atleast_2d(np.asarray(rows)).astype(T)
    with np.errstate(all="ignore"):
        exact = np.log(x.astype(HI))
        bound = _ulp(exact, T) + 4 * float(np.finfo(HI).eps) * np.abs(exact).astype(np.float64)
    return exact, bound


def fit_bound(rows, inv, T):
    """(exact, bound) of the coefficients: |got - exact| <= (n + m + 2) u sum_j |inv[k, j]| sum_i |w[i]| i**j + one ulp of T, u = 2**-53:
    n additions and one product behind every moment, m additions and a product in the matrix product, the conversion of i**j; the ulp is
    the rounding into T.  ``exact``: the same sums one precision up."""
    x = np.atleast_2d(np.asarray(rows)).astype(T).astype(HI)
    inv = np.asarray(inv, dtype=np.float64).astype(HI)
    m, n = len(inv), x.shape[1]
    powers = np.array([[HI(i**j) for j in range(m)] for i in range(n)])
    with np.errstate(all="ignore"):
        exact = (x @ powers) @ inv.T
        size = (np.abs(x) @ powers) @ np.abs(inv).T
        bound = ((n + m + 2) * U64 * size).astype(np.float64) + _ulp(exact, T)
    return exact, bound


def residual_bound(rows, pars, T, exp_rms):
    """(mean, rms, bound of mean, bound of rms): the sums of the residuals without any rounding, one precision up, and a running error
    bound of the written rounding sequence (the typing table): every float64 operation within u = 2**-53 of its exact result, every
    rounding into T within u_T, the two exponentials involved (NumPy's, the device's) within one ulp of float64 -- 2 u relative -- of
    exp of the argument they are given, whose own error dt multiplies the result by exp(+-dt).  The bound of each running sum grows by the
    error of the term added and by (u + u_T) of the new sum; the root's is the width of sqrt over [v - E, v + E].  First order terms of
    the bounds themselves are kept (E enters the sums they bound), nothing is dropped."""
    x = np.atleast_2d(np.asarray(rows)).astype(T).astype(HI)
    n_rows, n = x.shape
    p = np.broadcast_to(np.atleast_2d(np.asarray(pars)).astype(T), (n_rows, np.shape(pars)[-1])).astype(HI)
    m, uT = p.shape[1], unit(T)
    mean, rms, e_mean, e_rms = (np.zeros(n_rows, HI) for _ in range(4))
    with np.errstate(all="ignore"):
        for i in range(n):
            pw = [HI(i**j) for j in range(m)]
            temp = sum(p[:, j] * pw[j] for j in range(m))
            dt = (m + 2) * U64 * sum(np.abs(p[:, j]) * pw[j] for j in range(m))
            if exp_rms:
                e = np.exp(temp)
                de = e * (np.expm1(dt) + 2 * U64 * np.exp(dt))
                r = x[:, i] - e
                dr = de + U64 * (np.abs(r) + de)
            else:
                r = x[:, i] - temp
                dr = dt + U64 * (np.abs(r) + dt)
            q = r / (i + 1)
            dq = dr / (i + 1) + U64 * (np.abs(q) + dr / (i + 1))
            mean = mean + q
            e_mean = e_mean + dq + (U64 + uT) * (np.abs(mean) + e_mean + dq)
            s = r * r
            ds = 2 * np.abs(r) * dr + dr * dr
            ds = ds + U64 * (s + ds)
            rms = rms + s
            e_rms = e_rms + ds + (U64 + uT) * (rms + e_rms + ds)
        v = rms / (n - 1)
        e_v = e_rms / (n - 1)
        e_v = e_v + (U64 + uT) * (v + e_v)
        root = np.sqrt(v)
        e_root = np.sqrt(v + e_v) - np.sqrt(np.maximum(v - e_v, 0)) + uT * (root + e_v)
        tiny = n * float(np.finfo(T).tiny)  # (a rounding that lands among the subnormals)
        return mean, root, (e_mean + _ulp(mean, T) + tiny).astype(np.float64), (e_root + _ulp(root, T) + tiny).astype(np.float64)


def within(got, exact, bound, finite_of):
    """(ok, worst ratio): where the yardstick's own result ``finite_of`` is finite, |got - exact| <= bound; elsewhere got is the same
    infinity or a NaN as it"""
    got, finite_of = np.asarray(got), np.asarray(finite_of)
    fin = np.isfinite(finite_of)
    with np.errstate(all="ignore"):
        err = np.abs(got.astype(HI) - exact).astype(np.float64)
        ratio = np.where(fin, err / np.where(bound > 0, bound, 1.0), 0.0)
        ratio = np.where(fin & ~(err <= bound), np.inf, ratio)
    ok = bool(np.all(np.isfinite(ratio)) and np.all(ratio <= 1.0)) and same(np.where(fin, 0, got), np.where(fin, 0, finite_of))
    return ok, float(np.max(ratio)) if ratio.size else 0.0


# ---------------------------------------------------------------------------------------------------------------- the rows
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


FAMILIES = ("decay", "decay-fast", "small", "zero", "negative", "nan-first", "nan-middle", "nan-last", "inf")
BAD_FOR_LOG = ("zero", "negative", "nan-first", "nan-middle", "nan-last")
NAN_ROWS = ("nan-first", "nan-middle", "nan-last")


def tail_rows(loop, n):
    """a family per row (FAMILIES), in the loop's type: positive decaying exponentials with noise, and what log_check and the NaN rules are for"""
    rows = np.zeros((len(FAMILIES), n))
    f = FAMILIES.index
    rows[f("decay")] = _decay(n, 3000.0, 0.9996) + _draws(21 + n, n, -64, 64) / 8
    rows[f("decay-fast")] = _decay(n, 900.0, 0.97) + 20 + _draws(22 + n, n, -32, 32) / 16
    rows[f("small")] = (_decay(n, 5.0, 0.999) + _draws(23 + n, n, -8, 8) / 16) * 2.0**-20
    rows[f("zero")] = rows[f("decay")]
    rows[f("zero"), n // 2] = 0.0
    rows[f("negative")] = rows[f("decay")]
    rows[f("negative"), n - 1] = -3.5
    for name, at in (("nan-first", 0), ("nan-middle", n // 2), ("nan-last", n - 1)):
        rows[f(name)] = rows[f("decay")]
        rows[f(name), at] = np.nan
    rows[f("inf")] = rows[f("decay")]
    rows[f("inf"), n // 3] = np.inf
    return rows.astype(LOOPS[loop])


PAR_FAMILIES = ("tail", "log-tail", "flat", "wiggle", "nan", "overflow")


def coefficients(loop, m, n):
    """a set of m coefficients per family (PAR_FAMILIES), in the loop's type: the logarithm of ``decay`` and friends; the higher orders fall
    off with the row length so that every polynomial stays moderate; ``overflow``: exp(temp) leaves float64 from sample 10 on (where the
    row has one)"""
    scale = float(max(n, 2))
    sets = np.zeros((len(PAR_FAMILIES), m))
    f = PAR_FAMILIES.index
    sets[f("tail"), 0] = 8.0
    sets[f("log-tail"), 0] = 8.006
    sets[f("flat"), 0] = 2990.0
    sets[f("wiggle"), 0] = 7.5
    sets[f("nan"), 0] = 8.0
    sets[f("overflow"), 0] = 700.0
    for j in range(1, m):
        sets[f("tail"), j] = -0.4 / scale**j / j
        sets[f("log-tail"), j] = -0.0004 if j == 1 else 2.0**-30 / scale**j
        sets[f("flat"), j] = -1.2 if j == 1 else 0.25 / scale**j
        sets[f("wiggle"), j] = (-1.0) ** j * 0.75 / scale**j
        sets[f("nan"), j] = -0.1 / scale**j
        sets[f("overflow"), j] = 1.0 if j == 1 else 0.0
    sets[f("nan"), m - 1] = np.nan
    return sets.astype(LOOPS[loop])


def residual_case(loop, n, m):
    """every family of rows against every family of coefficients: (rows, pars), a set of coefficients per row"""
    rows, sets = tail_rows(loop, n), coefficients(loop, m, n)
    r, s = np.meshgrid(np.arange(len(rows)), np.arange(len(sets)), indexing="ij")
    return rows[r.reshape(-1)], sets[s.reshape(-1)]


def fit_cases():
    """(n, m) at which the factory's matrix can be inverted: a row holds at least as many samples as coefficients"""
    return [(n, m) for n in LENGTHS for m in MS if n >= m]


def tile_rows(a, count):
    """``count`` rows (or values) that repeat those of ``a`` in turn"""
    a = np.asarray(a)
    return a[np.arange(count) % len(a)]


# ---------------------------------------------------------------------------------------------------------------- programs
def program(n, rows=np.float32, loop=np.float32, log=False, fit=False, resid=None, resid_of="rows", m=4, store_log=True, store_pars=True, offset=0,
            row_stride=None, out_stride=None, out_len=None, pars_stride=None, subtract=None, inv_len=None, inv_dtype=np.float64):
    """LOAD, [LOAD of the coefficients,] [BL_SUBTRACT,] [LOG_CHECK,] [POLY_FIT,] [POLY_DIFF | POLY_EXP_RMS,] [STORE of the logged row,] [STORE of
    the coefficients,] [STORE_SCALAR, STORE_SCALAR]; ``resid``: "diff" or "exp"; ``resid_of``: "rows" or "log"; ``subtract``: a baseline, or
    "column" for one per event"""
    from dspeed_amd.chain import Program, Scalar

    p = Program()
    s_in = p.add_slot(n)
    p.add_op(_lib.OP_LOAD, dst=s_in, io=p.add_io("w", _lib.IO_WF_IN, rows, n, offset, row_stride))
    s_pars = None
    if resid and not fit:
        s_pars = p.add_slot(m)
        p.add_op(_lib.OP_LOAD, dst=s_pars, io=p.add_io("pars", _lib.IO_WF_IN, loop, m, 0, pars_stride))
    if subtract is not None:
        p.add_op(_lib.OP_BL_SUBTRACT, dst=s_in, src=s_in, sp=(Scalar.input(p.add_io("bl", _lib.IO_SCALAR_IN, loop)) if subtract == "column" else Scalar.const(subtract),))
    src = s_in
    if log:
        s_log = p.add_slot(n if out_len is None else out_len)
        p.add_op(_lib.OP_LOG_CHECK, dst=s_log, src=s_in)
        src = s_log
    if fit:
        s_pars = p.add_slot(m)
        p.add_op(_lib.OP_POLY_FIT, dst=s_pars, src=src, io=p.add_io("inv", _lib.IO_TAPS, inv_dtype, m * m if inv_len is None else inv_len, 0, 0))
    if resid:
        reg = p.add_sregs(2)
        p.add_op(_lib.OP_POLY_DIFF if resid == "diff" else _lib.OP_POLY_EXP_RMS, dst=reg, src=s_log if resid_of == "log" else s_in, ip=(s_pars,))
    if log and store_log:
        p.add_op(_lib.OP_STORE, src=s_log, io=p.add_io("out", _lib.IO_WF_OUT, loop, p.slots[s_log], 0, out_stride))
    if fit and store_pars:
        p.add_op(_lib.OP_STORE, src=s_pars, io=p.add_io("pars_out", _lib.IO_WF_OUT, loop, m, 0, None))
    if resid:
        p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io("mean", _lib.IO_SCALAR_OUT, loop), ip=(reg,))
        p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io("rms", _lib.IO_SCALAR_OUT, loop), ip=(reg + 1,))
    return p
