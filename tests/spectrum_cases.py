"""Cases of psd and fft (dsp_spectrum.hip): the rows that tools/gen_golden_spectrum.py feeds to the reference's bodies
(tests/golden/spectrum.npz holds what they returned), the error caps the tests hold every implementation to, and a NumPy model of the
kernel's formulation -- packing, radix-2 passes (natural order in, bit-reversed out), the unpacking step; Bluestein with the chirp's
j^2 reduced modulo 2 n in integers, the filter in bit-reversed order and the inverse passes with conjugate twiddles; the host tables in
float64 rounded once -- that test_spectrum_cases_cpu.py holds to the same rules before anything runs on a GPU.  Nothing here needs a GPU or
the reference.  Every row comes from a seed."""
import numpy as np

from dspeed_amd import _lib

BOOK = "spectrum"
KERNEL = "spectrum"
F32_POW2_MAX, F32_ANY_MAX = 16384, 4096   # dsp_program.h: DSP_SPECTRUM_F32_POW2_MAX / _ANY_MAX (the float64 loop: half of each)
WAVE_ROW_BYTES = 8 * 1024                 # dsp_kernels.h: a transform up to this size runs on a wavefront, a longer one on a workgroup
BASE = (1, 2, 3, 4, 5, 8, 16, 17, 20, 63, 64, 65, 127, 128, 255, 256, 257, 1000, 1024, 3000, 4096, 8192, 16384)
# either side of the wavefront / workgroup switch: float32 2048 | 4096 (packed) and 511 | 513 (Bluestein, 1024 | 2048 points); float64 1024 |
# 2048 and 255 | 257.  The largest other length admitted: 4095 (float32), 2047 (float64).
LENGTHS = tuple(sorted(BASE + (511, 513, 2048, 2047, 4095)))
LONG = 1024                               # rows longer than this: few per group
FLOAT_FAMILIES = ("noise", "pedestal", "pulse", "constant", "alternating", "delta0", "nan_first", "nan_mid", "nan_last", "inf_mid")
EXACT = ("constant", "alternating", "delta0")
CONSTANT, ALTERNATING = 3.0, 5.0
_ROW_TYPES = {"f32": np.float32, "f64": np.float64, "i16": np.int16, "u16": np.uint16}


def pow2(n):
    return n > 0 and n & (n - 1) == 0


def points(n):
    """complex points of a row's transform (dsp_kernels.h, dsp_spectrum::points)"""
    if pow2(n):
        return max(n // 2, 1)
    m = 1
    while m < 2 * n - 1:
        m *= 2
    return m


def wide(n, loop):
    return points(n) * 2 * np.dtype(loop).itemsize > WAVE_ROW_BYTES


def admitted(n, loop):
    half = 2 if np.dtype(loop) == np.float64 else 1
    return n <= (F32_POW2_MAX if pow2(n) else F32_ANY_MAX) // half


def eps(loop):
    return 2.0 ** -24 if np.dtype(loop) == np.float32 else 2.0 ** -53


def cap(n, loop):
    """rule 2: the L2 error of a spectrum relative to the float64 truth's norm -- eps log2 M, twice that through Bluestein's two transforms"""
    M = n if pow2(n) else points(n)
    return (1 if pow2(n) else 2) * eps(loop) * max(np.log2(M), 1.0)


def bar(n):
    """rule 4: the most a noise row's error may exceed the reference's float32 error on the same row"""
    return 8.0 if pow2(n) else 16.0


class Group:
    """Rows of one length and type that go through one launch: ``w`` (R, n) in the rows' own type, their families ``names``; ``stored``:
    the rows whose reference spectra the fixture holds (fft, and psd where ``with_psd``)."""

    def __init__(self, name, tag, rows, w, names, stored, with_psd):
        self.name, self.tag, self.rows, self.w, self.names, self.stored, self.with_psd = name, tag, rows, w, names, stored, with_psd
        self.loop = np.float32 if tag == "f32" else np.float64
        self.n = w.shape[1]

    def truth(self):
        """X64: NumPy's float64 rfft of the rows (NaN rows: whatever it makes of them; the rules do not look)"""
        with np.errstate(all="ignore"):
            return np.fft.rfft(self.w.astype(np.float64), axis=1)

    def finite(self):
        return np.isfinite(self.w.astype(np.float64)).all(axis=1)


def _row(family, n, rng):
    i = np.arange(n, dtype=np.float64)
    if family == "noise":
        return rng.normal(0.0, 5.0, n)
    if family == "pedestal":
        return 10000.0 + rng.integers(-20, 21, n)
    if family == "pulse":
        t0, amp, tau = n * rng.uniform(0.3, 0.6), rng.uniform(500, 15000), max(2.0, n / 3)
        return np.rint(10000.0 + rng.integers(-20, 21, n) + amp * np.exp(-np.maximum(i - t0, 0) / tau) * (i >= t0))
    if family == "constant":
        return np.full(n, CONSTANT)
    if family == "alternating":
        return ALTERNATING * (1 - 2 * (i % 2))
    if family == "delta0":
        return (i == 0).astype(np.float64)
    w = rng.normal(0.0, 5.0, n)
    w[{"nan_first": 0, "nan_mid": n // 2, "nan_last": n - 1, "inf_mid": n // 2}[family]] = np.inf if family == "inf_mid" else np.nan
    return w


def _families(n, rows):
    if rows == "f32" or rows == "f64":
        return FLOAT_FAMILIES if n <= LONG else ("noise", "pulse", "constant", "alternating")
    if rows == "i16":
        return ("noise", "pedestal", "pulse", "constant", "alternating", "delta0") if n <= LONG else ("noise", "pulse", "constant", "alternating")
    return ("pedestal", "pulse", "constant", "delta0")  # uint16


def _group(n, rows):
    rng = np.random.default_rng([20261020, n, sorted(_ROW_TYPES).index(rows)])
    names = list(_families(n, rows))
    w = np.array([_row(f, n, rng) for f in names])
    if rows == "i16":
        w = np.rint(w)
    w = w.astype(_ROW_TYPES[rows])
    tag = "f64" if rows == "f64" else "f32"
    if rows == "f64":  # the float64 loop's truth is NumPy's own: only the short rows' spectra are stored (the NaN rows' among them)
        stored = list(range(len(names))) if n <= 65 else []
    elif n <= LONG:
        stored = list(range(len(names)))
    else:
        stored = [names.index("noise")] if "noise" in names else []
    return Group(f"{rows}_n{n}", tag, rows, w, names, stored, with_psd=n <= 257)


def groups():
    """every group of the book, in a fixed order"""
    out = []
    for n in LENGTHS:
        for rows in ("f32", "f64") + (("i16",) if n in (65, 1000, 4096) else ()) + (("u16",) if n in (65, 1024) else ()):
            loop = np.float64 if rows == "f64" else np.float32
            if admitted(n, loop):
                out.append(_group(n, rows))
    return out


# ---------------------------------------------------------------------------------------------------------------- the tables, as the host makes them
def _unit(k, N):
    """exp(-2 pi i k / N) in float64; the multiples of a quarter turn exactly (dsp_spectrum_tables.h)"""
    k = np.asarray(k, dtype=np.int64) % N
    a = -2.0 * np.pi * k.astype(np.float64) / N
    re, im = np.cos(a), np.sin(a)
    quarter = (4 * k) % N == 0
    q = np.where(quarter, (4 * k) // N, 0)
    re = np.where(quarter, np.array([1.0, 0.0, -1.0, 0.0])[q], re)
    im = np.where(quarter, np.array([0.0, -1.0, 0.0, 1.0])[q], im)
    return re, im


def bit_reverse(L):
    bits = int(np.log2(L)) if L > 1 else 0
    p = np.arange(L)
    r = np.zeros(L, dtype=np.int64)
    for b in range(bits):
        r |= ((p >> b) & 1) << (bits - 1 - b)
    return r


def tables(n, T):
    """twiddle, aux (unpacking twiddles or chirp) and filter (Bluestein), each (re, im) of type T"""
    L = points(n)
    tw = _unit(np.arange(L // 2), max(L, 1))
    if pow2(n):
        aux, filt = _unit(np.arange(n // 2 + 1), n), None
    else:
        j = np.arange(n, dtype=np.int64)
        aux = _unit((j * j) % (2 * n), 2 * n)  # (integers: no angle is formed from j^2 itself)
        b = np.zeros(L, dtype=np.complex128)
        b[:n] = aux[0] - 1j * aux[1]
        b[L - np.arange(1, n)] = b[1:n]
        B = np.fft.fft(b)[bit_reverse(L)] / L
        filt = (B.real, B.imag)
    cast = lambda t: None if t is None else (t[0].astype(T), t[1].astype(T))  # noqa: E731
    return cast(tw), cast(aux), cast(filt)


# ---------------------------------------------------------------------------------------------------------------- the model
def _mul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def _forward(zr, zi, tw):
    L = len(zr)
    t = np.arange(L // 2)
    h, step = L // 2, 1
    while h >= 1:
        k = t & (h - 1)
        i = ((t - k) << 1) | k
        ar, ai, br, bi = zr[i], zi[i], zr[i + h], zi[i + h]
        zr[i], zi[i] = ar + br, ai + bi
        zr[i + h], zi[i + h] = _mul(ar - br, ai - bi, tw[0][k * step], tw[1][k * step])
        h, step = h // 2, step * 2


def _inverse(zr, zi, tw):
    L = len(zr)
    t = np.arange(L // 2)
    h, step = 1, L // 2
    while h < L:
        k = t & (h - 1)
        i = ((t - k) << 1) | k
        br, bi = _mul(zr[i + h], zi[i + h], tw[0][k * step], -tw[1][k * step])
        ar, ai = zr[i].copy(), zi[i].copy()
        zr[i], zi[i] = ar + br, ai + bi
        zr[i + h], zi[i + h] = ar - br, ai - bi
        h, step = h * 2, step // 2


def model_fft(row, T, tabs=None):
    """one row through the kernel's formulation in the arithmetic of T; complex result of n // 2 + 1 bins"""
    T = np.dtype(T).type
    n = len(row)
    m = n // 2 + 1
    C = np.complex64 if T is np.float32 else np.complex128
    x = np.asarray(row).astype(T)
    if not np.isfinite(x).all():
        return np.full(m, np.nan + 0j, dtype=C)
    if n == 1:
        return np.array([x[0] + 0j], dtype=C)
    tw, aux, filt = tabs or tables(n, T)
    L = points(n)
    with np.errstate(all="ignore"):
        if pow2(n):
            zr, zi = x[0::2].copy(), x[1::2].copy()
            _forward(zr, zi, tw)
            rev = bit_reverse(L)
            k = np.arange(m)
            pr, pi = zr[rev[k & (L - 1)]], zi[rev[k & (L - 1)]]
            qr, qi = zr[rev[(L - k) & (L - 1)]], zi[rev[(L - k) & (L - 1)]]
            half = T(0.5)
            er, ei, orr, oi = half * (pr + qr), half * (pi - qi), half * (pi + qi), half * (qr - pr)
            ur, ui = _mul(orr, oi, aux[0][k], aux[1][k])
            xr, xi = er + ur, ei + ui
            xr[0], xi[0] = er[0] + orr[0], T(0)
            xr[L], xi[L] = er[L] - orr[L], T(0)
        else:
            zr, zi = np.zeros(L, dtype=T), np.zeros(L, dtype=T)
            zr[:n], zi[:n] = x * aux[0], x * aux[1]
            _forward(zr, zi, tw)
            zr, zi = _mul(zr, zi, filt[0], filt[1])
            _inverse(zr, zi, tw)
            xr, xi = _mul(zr[:m], zi[:m], aux[0][:m], aux[1][:m])
    out = np.empty(m, dtype=C)
    out.real, out.imag = xr, xi
    return out


def model_psd(row, T):
    T = np.dtype(T).type
    X = model_fft(row, T)
    with np.errstate(all="ignore"):
        return ((X.real * X.real + X.imag * X.imag) / T(len(row))).astype(T)


# ---------------------------------------------------------------------------------------------------------------- the rules, for any implementation
def rel_l2(X, X64):
    d = np.linalg.norm(X.astype(np.complex128) - X64)
    return d / np.linalg.norm(X64)


def check_exact(name, n, X):
    """rule 1: power-of-two rows of the three families that multiply nothing but zeros by inexact twiddles"""
    want = np.zeros(n // 2 + 1, dtype=np.complex128)
    if name == "constant":
        want[0] = n * CONSTANT
    elif name == "alternating":
        want[n // 2 if n > 1 else 0] = n * ALTERNATING
    else:
        want[:] = 1.0
    assert np.array_equal(X.astype(np.complex128), want), (name, n, np.flatnonzero(X.astype(np.complex128) != want)[:5])


def check_nan(X, complex_out):
    """rule 5: every bin NaN -- fft: real part NaN, imaginary part 0"""
    if complex_out:
        assert np.isnan(X.real).all() and (X.imag == 0).all()
    else:
        assert np.isnan(X).all()


def check_psd(P, X, n, loop, P64, fft_cap):
    """rule 3: the power spectrum against the same implementation's fft, term by term, and against the truth in sum"""
    want = (X.real.astype(np.float64) ** 2 + X.imag.astype(np.float64) ** 2) / n
    assert (np.abs(P.astype(np.float64) - want) <= 4 * eps(loop) * want).all(), np.max(np.abs(P - want) / np.where(want > 0, want, 1))
    assert np.abs(P.astype(np.float64) - P64).sum() <= (2 * fft_cap + fft_cap ** 2) * P64.sum()


def check_group(g, case, X, P, what=""):
    """Rules 1 - 5 for what some implementation made of group ``g``'s rows: ``X`` (R, m) complex and ``P`` (R, m) real, in the loop's types;
    ``case``: the group's entry of the fixture.  Returns {row name: (error / cap, error / the reference's error or None)}."""
    C = np.complex64 if g.loop is np.float32 else np.complex128
    m = g.n // 2 + 1
    assert X.shape == (len(g.w), m) and X.dtype == C and P.shape == (len(g.w), m) and P.dtype == g.loop, (what, g.name, X.shape, X.dtype, P.shape, P.dtype)
    X64, finite, figures = g.truth(), g.finite(), {}
    stored = {r: k for k, r in enumerate(case.params["stored"])}
    for r, name in enumerate(g.names):
        tell = (what, g.name, name)
        if not finite[r]:  # rule 5
            check_nan(X[r], True)
            check_nan(P[r], False)
            if name != "inf_mid" and r in stored:  # (an infinity: the reference's mix of NaN and inf is the documented difference)
                ref = case["fft"][stored[r]]
                assert np.isnan(ref.real).all() and (ref.imag == 0).all(), tell
                if "psd" in case:
                    assert np.isnan(case["psd"][stored[r]]).all(), tell
            continue
        err, c = rel_l2(X[r], X64[r]), cap(g.n, g.loop)
        if pow2(g.n) and name in EXACT:  # rule 1
            check_exact(name, g.n, X[r])
            want = (X[r].real.astype(np.float64) ** 2 + X[r].imag.astype(np.float64) ** 2) / g.n
            assert np.array_equal(P[r].astype(np.float64), want), tell  # (9 n, 25 n, 1 / n: exact in either type)
        assert err <= c, (tell, err, c)  # rule 2
        P64 = (X64[r].real ** 2 + X64[r].imag ** 2) / g.n
        check_psd(P[r], X[r], g.n, g.loop, P64, c)  # rule 3
        ratio = None
        if name == "noise" and g.tag == "f32" and r in stored:  # rule 4
            ref_err = rel_l2(case["fft"][stored[r]], X64[r])
            if ref_err > 0:
                ratio = err / ref_err
                assert ratio <= bar(g.n), (tell, err, ref_err, ratio)
            else:
                assert err == 0, tell
        figures[name] = (err / c, ratio)
    return figures


# ---------------------------------------------------------------------------------------------------------------- programs, for the planner
def program(n, op="psd", rows=np.float32, loop=np.float32, offset=0, row_stride=None, bins=None):
    """LOAD, PSD | FFT, STORE"""
    from dspeed_amd.chain import Program

    p = Program()
    m = n // 2 + 1 if bins is None else bins
    width = 2 * m if op == "fft" else m
    s_in, s_out = p.add_slot(n), p.add_slot(width)
    p.add_op(_lib.OP_LOAD, dst=s_in, io=p.add_io("w", _lib.IO_WF_IN, rows, n, offset, row_stride))
    p.add_op(_lib.OP_FFT if op == "fft" else _lib.OP_PSD, dst=s_out, src=s_in)
    p.add_op(_lib.OP_STORE, src=s_out, io=p.add_io("out", _lib.IO_WF_OUT, loop, width))
    return p
