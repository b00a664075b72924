"""The case book of ``reflected_convolve_wf`` (dsp_reflect.hip), shared by the CPU and the GPU tests.  Not collected: a plain helper.

The yardstick is ``emulate``: the formula of the processor and the arithmetic of its loops restated in NumPy, line by line --

    out[i] = sum_{k=0}^{m-1} kernel[k] * w[r(i + (m-1)//2 - k)],   r(t) = -t below 0,  2 (n - 1) - t above n - 1,  t otherwise

with one float64 accumulator per output from +0, the products (double) w * (double) kernel[k] added in ascending k, one rounding at the
store.  In the float32 loop a product of two float32 values is exact in float64, so a NumPy loop of float64 multiplies and adds reproduces
a fused multiply-add bit for bit.  ``emulate`` itself is held to the reference body's recorded results (tests/golden/reflected_convolve.npz,
written by tools/gen_golden_reflect.py) in tests/test_reflect_cases_cpu.py; nothing of the code under test is its own yardstick.

A *pair* is (n, m): a row length and a tap count.  Every pair comes with every row family of the rows' type (``rows_of``) and two or three
kernels (``kernels_of``): an asymmetric integer kernel always -- a flipped kernel or a shifted centre shows on it --, and in turn Gaussian
weights from the generator, a kernel with a zero tap (under which one row holds a +inf) and a kernel with a NaN."""
import functools

import numpy as np

from dspeed_amd import _lib

KERNEL = "dsp_reflect_kernel"
BOOK = "reflected_convolve"
F32_MAX, F64_MAX = 16384, 8192  # DSP_REFLECT_*_MAX: len(w_in) + len(kernel) - 1 in the float32 / float64 loop
T = 2048  # the narrow / wide boundary in staged float32 samples (dsp_reflect::WAVE_ROW_BYTES / 4); the float64 loop: half
LOOPS = {"f32": np.float32, "i16": np.float32, "u16": np.float32, "f64": np.float64}
ROWS = {"f32": np.float32, "i16": np.int16, "u16": np.uint16, "f64": np.float64}
LIMITS = "len\\(w_in\\) \\+ len\\(kernel\\) - 1 of up to 16384 in the float32 loop and 8192 in the float64 loop"
ROW_COUNTS = (1, 3, 4, 5, 130)
LENGTHS = (1, 2, 3, 7, 8, 63, 64, 65, 255, 256, 257)
TAPS = (1, 2, 3, 4, 8, 9)
M_CAP = 257
INTEGER_M_MAX = 256  # |x| <= 2^11, |k| <= 2^4, m <= 2^8: every partial sum below 2^23, float32 summation exact in any order


def limit(rows):
    return F64_MAX if rows == "f64" else F32_MAX


def boundary(rows):
    return T // 2 if rows == "f64" else T


def wide(n, m, rows):
    return n + m - 1 > boundary(rows)


# ---------------------------------------------------------------------------------------------------------------- the rule and its wrong neighbours
def reflect(t, n):
    """r(t): one reflection, the edge sample not repeated"""
    return -t if t < 0 else 2 * (n - 1) - t if t > n - 1 else t


WRONG = ("symmetric", "centre", "unflipped", "short-margin", "one-edge")


def _source(i, k, n, m, variant):
    """(index of the sample tap k of output i multiplies, or None: the sample is missing and reads 0; index of the tap)"""
    c = m // 2 if variant == "centre" else (m - 1) // 2
    t = i + c - k
    tap = m - 1 - k if variant == "unflipped" else k
    if variant == "symmetric":  # numpy's "symmetric": the edge sample repeated
        src = -t - 1 if t < 0 else 2 * n - 1 - t if t > n - 1 else t
        return min(max(src, 0), n - 1), tap
    if variant == "centre":
        return min(max(reflect(t, n), 0), n - 1), tap
    if variant == "short-margin" and m >= 2 and t == -(m // 2):  # the outermost mirrored sample ahead of the row is not there
        return None, tap
    src = reflect(t, n)
    if variant == "one-edge" and t > n - 1 and 1 <= src <= m // 2:  # a sample both margins show went to the first only
        return None, tap
    return src, tap


def emulate(w, k, loop, variant=None):
    """``w`` (R, n) rows of any type, ``k`` the taps; ``loop``: np.float32 or np.float64.  ``variant``: one of WRONG, a wrong neighbour."""
    x = np.asarray(w).astype(loop)  # int16 / uint16 rows are widened first
    k = np.asarray(k, dtype=loop)
    R, n = x.shape
    m = len(k)
    assert 1 <= m <= n
    out = np.full((R, n), np.nan, dtype=loop)  # 1. w_out[:] = NaN
    if np.isnan(k).any():  # 2. a kernel with a NaN: every row
        return out
    i = np.arange(n)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(R):
            if np.isnan(x[r]).any():  # 2. a row with a NaN
                continue
            acc = np.zeros(n, dtype=np.float64)  # one float64 accumulator per output, from +0
            for j in range(m):  # ascending k
                if variant is None:
                    t = i + (m - 1) // 2 - j
                    sample = x[r, np.where(t < 0, -t, np.where(t > n - 1, 2 * (n - 1) - t, t))].astype(np.float64)
                    tap = j
                else:
                    src = [_source(q, j, n, m, variant) for q in range(n)]
                    tap = src[0][1]
                    sample = np.array([x[r, s] if s is not None else 0.0 for s, _ in src], dtype=np.float64)
                acc = acc + sample * np.float64(k[tap])  # (double) w * (double) kernel[k]
            out[r] = acc.astype(loop)  # rounded once at the store
    return out


def avg_current(g, length):
    """DSP_OP_AVG_CURRENT on the filtered rows ``g``: (g[k + L] - g[k]) / length in the loop's type; a row with a NaN: NaNs"""
    T_ = g.dtype.type
    L = int(length)
    with np.errstate(invalid="ignore", over="ignore"):
        out = ((g[:, L:] - g[:, :-L]).astype(g.dtype) / T_(length)).astype(g.dtype)
    out[np.isnan(g).any(axis=1)] = np.nan
    return out


# ---------------------------------------------------------------------------------------------------------------- pairs
def pairs(rows):
    """(n, m) of the book for a row type, every one inside the loop's limit"""
    out = []
    for n in LENGTHS:
        out += [(n, m) for m in sorted({*TAPS, n - 1, n}) if 1 <= m <= min(n, M_CAP)]
    b = boundary(rows)
    out += [(b - 1, 1), (b, 1), (b + 1, 1), (b - 9, 9), (b - 8, 9), (b - 7, 9)]  # n + m - 1 = boundary - 1, boundary, boundary + 1
    if rows != "f64":
        out.append((1024, 1024))
    lim = limit(rows)
    out += [(lim, 1), (lim - 8, 9), (lim - 256, 257)]  # n + m - 1 = the limit
    return out


def over_the_limit(rows):
    lim = limit(rows)
    return [(lim + 1, 1), (lim - 7, 9), (lim, 2)]


NAMED_PAIRS = [(1000, 9), (64, 64), (257, 8)]


# ---------------------------------------------------------------------------------------------------------------- kernels
def asymmetric(m):
    """integer taps in [-15, 15], no symmetry, never all zero"""
    return (((np.arange(m) * 7 + 3) % 31) - 15).astype(np.float64)


def gaussian(m, loop):
    """weights from the generator, for odd m: sigma = lw / 4 makes int(4 sigma + 0.5) = lw"""
    from dspeed_amd.processors import gaussian_filter1d

    lw = (m - 1) // 2
    k = np.empty(m, dtype=loop)
    gaussian_filter1d(loop(lw / 4 if lw else 0.1), loop(4), k)
    return k


def kernels_of(n, m, loop, index=0):
    """{name: taps in the loop's type} for a pair: 'asym' always, one of the others in turn"""
    ks = {"asym": asymmetric(m).astype(loop)}
    other = ("gauss", "zero", "nan")[index % 3]
    if other == "gauss" and m % 2 == 0:
        other = "zero"
    if other == "gauss":
        ks["gauss"] = gaussian(m, loop)
    elif other == "zero":
        z = asymmetric(m).astype(loop)
        z[m // 2] = 0
        ks["zero"] = z
    else:
        bad = asymmetric(m).astype(loop)
        bad[m // 2] = np.nan
        ks["nan"] = bad
    return ks


def integer_class(rows, n, m, name):
    """integer rows under integer taps, every partial sum below 2^23: exact in float32 in any order"""
    return name in ("asym", "zero") and m <= INTEGER_M_MAX


# ---------------------------------------------------------------------------------------------------------------- rows
INT_FAMILIES = ("ramp", "spike-0", "spike-1", "spike-n-2", "spike-n-1", "pedestal")
FLOAT_FAMILIES = INT_FAMILIES + ("nan-first", "nan-middle", "nan-last", "inf")


def families(rows):
    return FLOAT_FAMILIES if rows in ("f32", "f64") else INT_FAMILIES


def _family(name, n, rows, rng):
    signed = rows != "u16"
    if name == "ramp":
        return (np.arange(n) % 1024) - (512 if signed else 0)
    if name.startswith("spike-"):
        at = {"0": 0, "1": min(1, n - 1), "n-2": max(n - 2, 0), "n-1": n - 1}[name[6:]]
        w = np.full(n, 3)
        w[at] = 1000
        return w
    if name == "pedestal":  # noise on a pedestal of 2000, as histogram_cases.sipm_rows has it
        return 2000 + np.rint(4 * rng.standard_normal(n))
    w = np.rint(100 * rng.uniform(-1, 1, n))
    if name == "inf":
        w[n // 2] = np.inf
    else:
        w[{"nan-first": 0, "nan-middle": n // 2, "nan-last": n - 1}[name]] = np.nan
    return w


def rows_of(rows, n):
    """(R, n) in the rows' type: one row per family; integer-valued, |x| <= 2^11, but for the NaN and the +inf"""
    rng = np.random.default_rng(0xEF1 + n)
    fams = families(rows)
    with np.errstate(invalid="ignore"):
        return np.stack([np.asarray(_family(f, n, rows, rng), dtype=np.float64) for f in fams]).astype(ROWS[rows])


def finite_rows(rows):
    return [i for i, f in enumerate(families(rows)) if not f.startswith("nan") and f != "inf"]


@functools.lru_cache(maxsize=None)
def want(rows, n, m, name, index=0):
    """the emulation of a case, computed once (read it, do not write to it)"""
    return emulate(rows_of(rows, n), kernels_of(n, m, LOOPS[rows], index)[name], LOOPS[rows])


def cases(rows):
    """(index, n, m, name of the kernel, its taps) over the whole book"""
    for index, (n, m) in enumerate(pairs(rows)):
        for name, k in kernels_of(n, m, LOOPS[rows], index).items():
            yield index, n, m, name, k


# ---------------------------------------------------------------------------------------------------------------- the fixture's part
FIXTURE_LENGTHS = (1, 2, 3, 7, 8, 63, 64, 65)
GAUSS = ((1, 4), (0.5, 4), (2.5, 3), (10, 4))  # (sigma, truncate) of the generator's fixture


def fixture_pairs():
    out = []
    for n in FIXTURE_LENGTHS:
        out += [(n, m) for m in sorted({*TAPS, n - 1, n}) if 1 <= m <= n]
    return out + [(257, 9), (256, 256), (257, 257), (1000, 9)]


def fixture_cases(loop_name):
    """(key, n, m, name, taps) of the fixture in a loop ('f32' / 'f64'): the rows are rows_of(loop_name, n)"""
    for index, (n, m) in enumerate(fixture_pairs()):
        for name, k in kernels_of(n, m, LOOPS[loop_name], index).items():
            yield f"{loop_name}_n{n}_m{m}_{name}", n, m, name, k


# ---------------------------------------------------------------------------------------------------------------- programs
def program(n, m, rows=np.float32, loop=np.float32, offset=0, row_stride=None, out_stride=None, out_len=None, lag=0, store_row=True, taps_len=None,
            length=None):
    """LOAD, REFLECTED_CONVOLVE, STORE; with ``lag``: LOAD, REFLECTED_CONVOLVE, AVG_CURRENT, STORE of the current [, STORE of the filtered row]"""
    from dspeed_amd.chain import Program, Scalar

    p = Program()
    p_len = n if out_len is None else out_len
    s_in, s_out = p.add_slot(n), p.add_slot(p_len)
    p.add_op(_lib.OP_LOAD, dst=s_in, io=p.add_io("w", _lib.IO_WF_IN, rows, n, offset, row_stride))
    p.add_op(_lib.OP_REFLECTED_CONVOLVE, dst=s_out, src=s_in, io=p.add_io("taps:k", _lib.IO_TAPS, loop, m if taps_len is None else taps_len, 0, 0))
    if lag:
        s_cur = p.add_slot(p_len - lag)
        p.add_op(_lib.OP_AVG_CURRENT, dst=s_cur, src=s_out, sp=(Scalar.const(float(lag if length is None else length)),))
        p.add_op(_lib.OP_STORE, src=s_cur, io=p.add_io("curr", _lib.IO_WF_OUT, loop, p_len - lag, 0, None))
    if store_row or not lag:
        p.add_op(_lib.OP_STORE, src=s_out, io=p.add_io("out", _lib.IO_WF_OUT, loop, p_len, 0, out_stride))
    return p
