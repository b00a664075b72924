"""The case book of ``interpolating_upsampler`` (dsp_interp.hip), shared by the CPU and the GPU tests.  Not collected: a plain helper.

``emulate`` is the yardstick: the reference's body (processors/upsampler.py:105-216) restated loop for loop -- the same walks over the
INPUT samples, the same float64 bound expressions, the same operation order -- under numba's typing of the float32 loop:
  * u, t, the polynomial weights and the spline's u / w2 arrays are float64;
  * float32 (op) float32 stays float32: a_next - a, w[1] - w[0], w[-1] - w[-2], w[i+1] - w[i-1], w[i+2] - w[i] are rounded to float32 first;
  * everything they then meet is float64, the store rounds to float32;
  * the spline's w[i+1] - 2 w[i] + w[i-1] is float64 throughout (int64 * float32 is float64);
  * x**3 with a literal exponent is numba's unrolled product x * (x * x), x**2 is x * x.
It works on a block of rows at once (nothing of the index arithmetic depends on the row), and its two deviations from the body are the ones
the device makes: the store at w_out[len(w_out)] of mode 's' is not made, and mode 'i' truncates its float slice bound.  With
``powers="libm"`` the powers are C's pow, which is what the body computes when CPython runs it: that variant is held bit for bit to the
fixture the reference's own body wrote (tests/golden/interp_upsampler.npz, tests/test_interp_cases_cpu.py), the numba variant is what the
device is held to.

A *case* is a block of rows of one type and length n, resampled to m samples in every mode the pair allows."""
import functools
import math
import os

import numpy as np

from dspeed_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "dsp_interp_kernel"
MODES = "infclhs"
LOOPS = {"f32": np.float32, "i16": np.float32, "u16": np.float32, "f64": np.float64}
ROWS = {"f32": np.float32, "i16": np.int16, "u16": np.uint16, "f64": np.float64}
WARM, STATIONARY = 48, 15  # dsp_interp::WARM, STATIONARY of dsp_kernels.h (tests/test_interp_plan_cpu.py reads them there)
WAVE_ROW_BYTES = 8 * 1024  # dsp_interp::WAVE_ROW_BYTES: the longest row a wavefront takes alone
LIMITS = "rows of up to 16384 samples in the float32 loop and 8192 in the float64 loop"
SPLINE_LIMITS = "mode 's' takes rows of up to 5456 samples in the float32 loop and 4096 in the float64 loop"


def limit(mode, rows):
    f64 = rows == "f64"
    if mode == "s":
        return _lib.INTERP_SPLINE_F64_MAX if f64 else _lib.INTERP_SPLINE_F32_MAX
    return _lib.INTERP_F32_MAX // (2 if f64 else 1)


def row_bytes(mode, n, esz):
    r16 = lambda b: (b + 15) // 16 * 16  # noqa: E731
    return r16(n * esz) + (r16(n * 8) if mode == "s" else 0)


def wide(mode, n, esz):
    return row_bytes(mode, n, esz) > WAVE_ROW_BYTES


def modes_of(n, m):
    """the modes a pair allows: 'i' wants a multiple, 'h' two samples"""
    return "".join(c for c in MODES if not (c == "i" and m % n) and not (c == "h" and n < 2))


# ---------------------------------------------------------------------------------------------------------------- the emulation
def _pow_numba(x, k):
    return x * x if k == 2 else x * (x * x)


def _pow_libm(x, k):
    return np.array([math.pow(v, k) for v in np.asarray(x, dtype=np.float64).ravel()], dtype=np.float64).reshape(np.shape(x))


def emulate(w, mode, m, powers="numba"):
    """w: (R, n) rows in the loop's type (float32 or float64); returns (R, m) in that type"""
    T = w.dtype.type
    assert T in (np.float32, np.float64) and w.ndim == 2
    P = _pow_numba if powers == "numba" else _pow_libm
    R, n = w.shape
    out = np.full((R, m), np.nan, dtype=T)
    ok = ~np.isnan(w).any(axis=1)
    f = w.astype(np.float64)  # (exact)
    up = m / n
    o_all = np.arange(m, dtype=np.float64)
    res = np.full((R, m), np.nan, dtype=T)
    with np.errstate(all="ignore"):
        if mode == "i":
            assert up == int(up)
            for i in range(n):
                o = int(up * i)
                res[:, o] = w[:, i]
                res[:, o + 1:int(o + up)] = 0
        elif mode in "nc":
            last = 0
            for i in range(n):
                nxt = math.ceil(up * (i + 0.5)) if mode == "n" else math.floor(up * i) + 1
                res[:, last:nxt] = w[:, i:i + 1]
                last = nxt
            res[:, last:] = w[:, n - 1:n]
        elif mode == "f":
            last = 0
            for i in range(n):
                nxt = math.ceil(up * (i + 1))
                res[:, last:nxt] = w[:, i:i + 1]
                last = nxt
        elif mode == "l":
            last = 0
            for i in range(n):
                nxt = math.ceil(up * (i + 1))
                a, a_next = w[:, i:i + 1], w[:, min(i + 1, n - 1):min(i + 1, n - 1) + 1]
                if nxt > last:
                    t = o_all[last:min(nxt, m)] / up - i
                    res[:, last:nxt] = (a.astype(np.float64) + t * (a_next - a).astype(np.float64)).astype(T)
                last = nxt
        elif mode == "h":
            assert n >= 2

            def segment(i, lo, hi):
                m0 = (w[:, 1] - w[:, 0]).astype(np.float64) if i == 0 else (w[:, i + 1] - w[:, i - 1]).astype(np.float64) / 2
                m1 = (w[:, -1] - w[:, -2]).astype(np.float64) if i == n - 2 else (w[:, i + 2] - w[:, i]).astype(np.float64) / 2
                t0 = o_all[lo:hi] / up - i
                t1 = 1 - t0
                v = ((-2 * P(t1, 3) + 3 * P(t1, 2)) * f[:, i:i + 1] + (-2 * P(t0, 3) + 3 * P(t0, 2)) * f[:, i + 1:i + 2]
                     - (P(t1, 3) - P(t1, 2)) * m0[:, None] + (P(t0, 3) - P(t0, 2)) * m1[:, None])
                res[:, lo:hi] = v.astype(T)

            last = 0
            for i in range(n - 1):
                nxt = math.ceil(up * (i + 1))
                if min(nxt, m) > last:
                    segment(i, last, min(nxt, m))
                last = nxt
            if m > last:
                segment(n - 2, last, m)
        elif mode == "s":
            u = np.zeros((R, n))
            w2 = np.zeros((R, n))
            for i in range(1, n - 1):
                p = 0.5 * w2[:, i - 1] + 2
                w2[:, i] = -0.5 / p
                u[:, i] = f[:, i + 1] - 2 * f[:, i] + f[:, i - 1]
                u[:, i] = (3 * u[:, i] - 0.5 * u[:, i - 1]) / p
            last = m
            for i in range(n - 2, -1, -1):
                w2[:, i] = w2[:, i] * w2[:, i + 1] + u[:, i]
                nxt = math.ceil(up * i)
                lo, hi = nxt, min(last, m - 1)  # (the store at m is not made)
                if hi >= lo:
                    t0 = o_all[lo:hi + 1] / up - i
                    t1 = 1 - t0
                    v = (t1 * f[:, i:i + 1] + t0 * f[:, i + 1:i + 2]
                         + ((P(t1, 3) - t1) * w2[:, i:i + 1] + (P(t0, 3) - t0) * w2[:, i + 1:i + 2]) / 6.0)
                    res[:, lo:hi + 1] = v.astype(T)
                last = nxt
        else:
            raise ValueError(mode)
    out[ok] = res[ok]
    return out


# ---------------------------------------------------------------------------------------------------------------- the kernel's formulation
def bounds(mode, n, m):
    """bound(i): the first output that input sample i does not fill, as dsp_interp::bound computes it (one multiply, one rounding)"""
    up = m / n
    i = np.arange(n, dtype=np.float64)
    if mode == "n":
        return np.ceil(up * (i + 0.5)).astype(np.int64)
    if mode == "c":
        return np.floor(up * i).astype(np.int64) + 1
    return np.ceil(up * (i + 1)).astype(np.int64) + (1 if mode == "s" else 0)


def rational_bounds(mode, n, m):
    """the same bounds in exact arithmetic: what the reference does NOT compute"""
    i = np.arange(n, dtype=object)
    if mode == "n":
        return np.array([-((-(m * (2 * k + 1))) // (2 * n)) for k in i], dtype=np.int64)
    if mode == "c":
        return np.array([m * k // n + 1 for k in i], dtype=np.int64)
    return np.array([-((-(m * (k + 1))) // n) for k in i], dtype=np.int64) + (1 if mode == "s" else 0)


def spline_w2(f, G, warm=WARM):
    """the second derivatives as the kernel makes them: G threads, each a chunk of an odd number of neighbouring samples, u from a warm-up
    of `warm` samples and the back substitution from one on the far side; a row with an infinity: the two sweeps in order"""
    R, n = f.shape
    w2 = np.zeros((R, n))
    if n < 3:
        return w2
    coef = np.zeros(n)
    for i in range(1, n - 1):
        coef[i] = -0.2679491924311227 if i >= STATIONARY else -0.5 / (0.5 * coef[i - 1] + 2.0)
    d = np.zeros((R, n))
    d[:, 1:-1] = (f[:, 2:] - 2.0 * f[:, 1:-1]) + f[:, :-2]
    p = np.full(n, 2.0)
    p[1:] = 0.5 * coef[:-1] + 2.0  # p[i] = 0.5 w2[i - 1] + 2 of the forward sweep
    L = ((n + G - 1) // G) | 1
    u = np.zeros((R, n))
    chunks = []
    for tid in range(G):
        a, b = tid * L, min(tid * L + L, n)
        lo, hi = max(a, 1), min(b, n - 1)
        if lo < hi:
            chunks.append((lo, hi))
    with np.errstate(all="ignore"):
        for lo, hi in chunks:
            s = max(lo - warm, 1)
            uu = np.zeros(R)
            for i in range(s, hi):
                uu = (3.0 * d[:, i] - 0.5 * uu) / p[i]
                if i >= lo:
                    u[:, i] = uu
        for lo, hi in chunks:
            W = np.zeros(R)
            if hi < n - 1:
                e = min(hi + warm, n - 1)
                for i in range(e - 1, hi - 1, -1):
                    W = coef[i] * W + u[:, i]
            for i in range(hi - 1, lo - 1, -1):
                W = coef[i] * W + u[:, i]
                w2[:, i] = W
        inf = np.isinf(f).any(axis=1)
        if inf.any():
            g = f[inf]
            uu, us = np.zeros(len(g)), np.zeros((len(g), n))
            for i in range(1, n - 1):
                uu = (3.0 * ((g[:, i + 1] - 2.0 * g[:, i]) + g[:, i - 1]) - 0.5 * uu) / p[i]
                us[:, i] = uu
            W = np.zeros(len(g))
            ws = np.zeros((len(g), n))
            for i in range(n - 2, -1, -1):
                W = coef[i] * W + us[:, i]
                ws[:, i] = W
            w2[inf] = ws
    return w2


def model(w, mode, m, variant=None, warm=WARM):
    """The kernel's formulation in NumPy: every OUTPUT looks its segment up (the smallest i with o < bound(i)), the spline's second
    derivatives come from warm-up sweeps.  ``variant`` names a wrong neighbour the case book must catch."""
    T = w.dtype.type
    R, n = w.shape
    f = w.astype(np.float64)
    up = m / n
    o = np.arange(m, dtype=np.int64)
    of = o.astype(np.float64)
    B = rational_bounds(mode, n, m) if variant == "rational" else None
    with np.errstate(all="ignore"):
        if mode == "i":
            r = m // n
            res = np.where((o % r == 0)[None, :], w[:, o // r], T(0))
        else:
            if B is None:
                B = bounds(mode, n, m)
            seg = np.searchsorted(B, o, side="right")  # the smallest i with o < B[i]; n: none
            if mode in "nc":
                res = w[:, np.minimum(seg, n - 1)]
            elif mode == "f":
                res = np.where((seg < n)[None, :], w[:, np.minimum(seg, n - 1)], T(np.nan))
            elif mode == "l":
                i = np.minimum(seg, n - 1)
                a, a_next = w[:, i], w[:, np.minimum(i + 1, n - 1)]
                t = of / up - i
                diff = (f[:, np.minimum(i + 1, n - 1)] - f[:, i]) if variant == "l-diff-f64" else (a_next - a).astype(np.float64)
                res = np.where((seg < n)[None, :], (a.astype(np.float64) + t * diff).astype(T), T(np.nan))
            elif mode == "h":
                i = np.minimum(seg, n - 2)
                t0 = of / up - i
                if variant == "h-tail-clamped":
                    t0 = np.where(seg > n - 2, np.minimum(t0, 1.0), t0)
                t1 = 1 - t0
                m0 = np.where((i == 0)[None, :], (w[:, 1:2] - w[:, 0:1]).astype(np.float64), (w[:, i + 1] - w[:, np.maximum(i - 1, 0)]).astype(np.float64) / 2)
                m1 = np.where((i == n - 2)[None, :], (w[:, -1:] - w[:, -2:-1]).astype(np.float64), (w[:, np.minimum(i + 2, n - 1)] - w[:, i]).astype(np.float64) / 2)
                t1_2, t0_2 = t1 * t1, t0 * t0
                t1_3, t0_3 = t1 * t1_2, t0 * t0_2
                res = ((((-2.0 * t1_3 + 3.0 * t1_2) * f[:, i] + (-2.0 * t0_3 + 3.0 * t0_2) * f[:, i + 1]) - (t1_3 - t1_2) * m0) + (t0_3 - t0_2) * m1).astype(T)
            else:
                if n < 2:
                    res = np.full((R, m), np.nan, dtype=T)
                else:
                    if variant == "s-upper-segment":
                        seg = np.searchsorted(B - 1, o, side="right")  # a bound goes to the segment above
                    i = np.minimum(seg, n - 2)
                    w2 = spline_w2(f, 256 if wide("s", n, w.dtype.itemsize) else 64, warm)
                    t0 = of / up - i
                    t1 = 1 - t0
                    t1_3, t0_3 = t1 * (t1 * t1), t0 * (t0 * t0)
                    res = ((t1 * f[:, i] + t0 * f[:, i + 1]) + ((t1_3 - t1) * w2[:, i] + (t0_3 - t0) * w2[:, i + 1]) / 6.0).astype(T)
    out = np.full((R, m), np.nan, dtype=T)
    ok = ~np.isnan(w).any(axis=1)
    out[ok] = np.asarray(res, dtype=T)[ok]
    return out


# ---------------------------------------------------------------------------------------------------------------- the rows
FLOAT_FAMILIES = ("noise", "pulse", "constant", "alternating", "spike", "integers", "nan-first", "nan-middle", "nan-last",
                  "+inf-first", "-inf-middle", "+inf-last", "-inf-first", "+inf-middle", "-inf-last")
INT_FAMILIES = ("noise", "pulse", "constant", "alternating", "spike", "integers", "extremes")


def _family(name, n, dt, rng):
    i = np.arange(n)
    integer = np.issubdtype(dt, np.integer)
    ped = 1000.0 if np.dtype(dt) != np.dtype(np.int16) else -500.0
    if name == "noise":
        w = ped + 5.0 * rng.standard_normal(n)
    elif name == "pulse":
        w = ped + 3000.0 * (i >= n // 3) * np.exp(-np.maximum(i - n // 3, 0) / max(n / 4.0, 1.0)) + 2.0 * rng.standard_normal(n)
    elif name == "constant":
        w = np.full(n, ped + 0.25)
    elif name == "alternating":
        w = np.where(i % 2 == 0, 7.5, -3.25) + ped
    elif name == "spike":
        w = ped + rng.standard_normal(n)
        w[n // 2] += 1.0e4
    elif name == "integers":
        w = rng.integers(-2000, 2000, n).astype(np.float64) + (4000 if np.dtype(dt) == np.dtype(np.uint16) else 0)
    elif name == "extremes":
        info = np.iinfo(dt)
        return rng.choice(np.array([info.min, info.min + 1, 0, info.max - 1, info.max], dtype=dt), n)
    else:
        kind, where = name.rsplit("-", 1)
        w = ped + 5.0 * rng.standard_normal(n)
        w[{"first": 0, "middle": n // 2, "last": n - 1}[where]] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[kind]
    return np.rint(w).astype(dt) if integer else w.astype(dt)


@functools.lru_cache(maxsize=None)
def rows_of(rows, n):
    """the block of a type and length: one row per family"""
    dt = ROWS[rows]
    rng = np.random.default_rng([n, sorted(ROWS).index(rows)])
    fams = INT_FAMILIES if rows in ("i16", "u16") else FLOAT_FAMILIES
    w = np.stack([_family(name, n, dt, rng) for name in fams])
    w.setflags(write=False)
    return w


def integer_rows_of(n):
    """integer-valued rows below 2^23 as float32: where the float32 loop is the body run on a float64 copy with one rounding at the store"""
    rng = np.random.default_rng([n, 99])
    w = np.stack([_family(name, n, np.int16, rng).astype(np.float32) for name in ("noise", "pulse", "alternating", "spike", "integers")])
    return w


# ---------------------------------------------------------------------------------------------------------------- lengths and ratios
def _first_float_bound_pair(mode):
    """the first (n, m), n < 40, whose float64 bound differs from the rational one at an interior index: the book's own search"""
    for n in range(3, 40):
        for m in range(n + 1, 6 * n):
            d = np.flatnonzero(bounds(mode, n, m) != rational_bounds(mode, n, m))
            if len(d) and 0 < d[0] < n - 1:
                return n, m
    raise AssertionError(mode)


FLOAT_BOUND_PAIRS = {mode: _first_float_bound_pair(mode) for mode in "nfc"}
NAMED_PAIRS = [(14, 58), (7, 58), (18, 150)]
SMALL = [1, 2, 3, 4, 5, 15, 16, 17, 47, 48, 49, 50, 51, 63, 64, 65, 127, 128, 129, 255, 256, 257]
# both sides of the narrow / wide switch of each loop and mode group, 16 N - 1 / 16 N for the loader, two lengths of several chunks a lane
SWITCH = {"f32": [682, 683, 2048, 2049], "f64": [512, 513, 1024, 1025]}
LOADER = [1023, 1024, 3071, 3072]


def _ms(n, k):
    """the ratios a length is tried with: every length gets three of the list, in turn"""
    every = [n, 2 * n, 10 * n, 16 * n, n - 1, n + 1, 1, (3 * n + 1) // 2, (7 * n) // 3, max(n // 2, 1), max(4 * n // 9, 1)]
    big = n > 600
    pick = [every[(k + j * 4) % len(every)] for j in range(3)]
    return sorted({m for m in pick if m >= 1 and not (big and m > 3 * n)} | ({2 * n} if k % 2 == 0 else {n + 1}))


@functools.lru_cache(maxsize=None)
def pairs(rows):
    """the (n, m) of a type"""
    if rows == "f32":
        ns = SMALL + SWITCH["f32"] + LOADER
    elif rows == "f64":
        ns = SMALL[::2] + SWITCH["f64"] + LOADER[:2]
    else:
        ns = [1, 2, 5, 16, 17, 63, 64, 129, 255, 683, 1024, 3071]
    out = []
    for k, n in enumerate(ns):
        out += [(n, m) for m in _ms(n, k)]
    out += NAMED_PAIRS + sorted(set(FLOAT_BOUND_PAIRS.values()))
    if rows in ("f32", "f64"):  # each limit and the sample below it, at a ratio that keeps the output short
        top, top_s = limit("l", rows), limit("s", rows)
        out += [(top, top + 1), (top - 1, 2 * (top - 1)), (top_s, top_s + 3), (top_s - 1, top_s - 2)]
    return list(dict.fromkeys(out))


@functools.lru_cache(maxsize=None)
def want(rows, n, m, mode):
    """the emulation's answer for the block of (rows, n), in the loop's type: computed once, shared, read-only"""
    out = emulate(rows_of(rows, n).astype(LOOPS[rows]), mode, m)
    out.setflags(write=False)
    return out


def modes_for(rows, n, m):
    return "".join(c for c in modes_of(n, m) if n <= limit(c, rows))


# ---------------------------------------------------------------------------------------------------------------- the program
def program(n, m, mode="l", rows=np.float32, loop=np.float32, offset=0, row_stride=None, out_stride=None, out_len=None):
    """LOAD, INTERP_UPSAMPLE, STORE"""
    from dspeed_amd.chain import Program

    p = Program()
    s_in, s_out = p.add_slot(n), p.add_slot(m)
    p.add_op(_lib.OP_LOAD, dst=s_in, io=p.add_io("w", _lib.IO_WF_IN, rows, n, offset, row_stride))
    p.add_op(_lib.OP_INTERP_UPSAMPLE, dst=s_out, src=s_in, ip=(ord(mode) if isinstance(mode, str) else mode,))
    p.add_op(_lib.OP_STORE, src=s_out, io=p.add_io("out", _lib.IO_WF_OUT, loop, m if out_len is None else out_len, 0, out_stride))
    return p


# ---------------------------------------------------------------------------------------------------------------- the fixture's part of the book
BOOK = "interp_upsampler"
FIXTURE_F64_ROWS = ("noise", "pulse", "nan-middle", "+inf-middle")


def fixture_pairs():
    """the pairs the reference's own body is run on (tools/gen_golden_interp.py): the short outputs of the float64 book, the named pairs and
    the searched ones -- the pure-Python body and the size of a committed file set the bound"""
    return [(n, m) for n, m in dict.fromkeys(pairs("f64") + pairs("f32")) if m <= 66 or (n, m) in NAMED_PAIRS or (n, m) in FLOAT_BOUND_PAIRS.values() or (n in (49, 129) and m <= 130)]


def fixture_rows(loop, n):
    """float64 loop: rows of the float64 block; float32 loop: integer-valued rows"""
    if loop == "f64":
        return rows_of("f64", n)[[FLOAT_FAMILIES.index(k) for k in FIXTURE_F64_ROWS]]
    return integer_rows_of(n)[[0, 1, 3]]
