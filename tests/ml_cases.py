"""The case book of the neural-network layers (dsp_dense.hip; reference processors/ml.py) and an emulation of the DEVICE's rule:

* every output is one fused multiply-add chain in ascending k from +0 -- ``tests/ml_fma.cpp``, a host program with ``fmaf`` / ``fma``
  (Python 3.10 has no ``math.fma``; a float64 product-and-add rounded twice is another function);
* the bias is added behind the chain, one addition of the loop's type;
* the activation follows numba's typing of the reference's own nopython gufuncs (``typing="numba"``): in the float32 loop ``np.exp`` of a
  float32 array is float32, ``0.01 * x_in``, ``1 + np.exp(..)`` and ``1 / (..)`` are float64, the store rounds once.  ``typing="numpy2"`` is
  what CPython with NumPy 2 computes for the same lines (a Python float beside a float32 array stays float32): the fixture
  ``tests/golden/ml_layers.npz`` records the reference body's result under it.
* ``normalisation_layer``: ``(x - means) / sqrt(variances)``, every step in the loop's type.

The bars (the issue's): bit for bit against this emulation for 'r' and 'l' in the float32 loop; bit for bit against the reference body on
integer-valued rows and weights whose partial sums stay below 2^24 (``fixture_*``); and for every activation, against the float64
(float64 loop: long double) evaluation of the reference body, ``bound``:

    |device - exact| <= L (n + 2) u (sum_i |x_i w_ij| + |b_j|) + act_ulps ulp(exact)

u = 2^-24 / 2^-53, L = 1 for r l m t and 1/4 for s: the standard bound of a dot product in any order (NumPy's own np.dot meets it:
tests/test_ml_cases_cpu.py), carried through an activation of Lipschitz constant L.
"""
import functools
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "dsp_dense_kernel"
BOOK = "ml_layers"
N_MAX, M_MAX = 16384, 256
LIMITS = "layers of up to 16384 inputs and 256 outputs"
ACTIVATIONS = "srlmt"
UNKNOWN = "q"  # an activation character the reference does not know: NaN outputs, no error
LOOPS = {"f32": np.float32, "i16": np.float32, "u16": np.float32, "f64": np.float64}
ROWS = {"f32": np.float32, "i16": np.int16, "u16": np.uint16, "f64": np.float64}
U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
LIPSCHITZ = {"r": 1.0, "l": 1.0, "m": 1.0, "t": 1.0, "s": 0.25}

# The activation term of the bound, in ulps of the loop's type at the exact value.  MEASURED_ACT_ULPS: measured on the CPU over the book's
# pre-activations (``activation_distances``; tests/test_ml_cases_cpu.py prints the figures and holds them against this table) -- the largest
# distance between the reference body's output in the loop's type (numba's typing, NumPy's own exp, tanh, log) and the evaluation of the
# same pre-activation one precision up, rounded up to two digits:
#   float32 loop   s 2.59   m 2.43   t 1.36
#   float64 loop   s 1.99   m 62591  t 1.16      (r and l: 0, exact operations of an exact argument)
# The float64 loop's softplus is the expression as written, log(1 + exp(x)): 1 + exp(x) rounds away most of exp(x) for x << 0 (the book
# reaches x = -8), in the reference as on the device; in the float32 loop that sum is a float64.  The device's exp / tanh / log are another
# library's: it gets FACTOR = 2 times the measured distance and never less than 2 ulp.
MEASURED_ACT_ULPS = {"f32": {"s": 2.6, "m": 2.5, "t": 1.4, "r": 0.0, "l": 0.0}, "f64": {"s": 2.0, "m": 62600.0, "t": 1.2, "r": 0.0, "l": 0.0}}
FACTOR = 2.0


def act_ulps(T, act):
    return max(FACTOR * MEASURED_ACT_ULPS["f64" if np.dtype(T) == np.float64 else "f32"][act], 2.0)


def chunk(loop):
    """samples of a row staged at a time (dsp_kernels.h, dsp_dense::chunk): 256 bytes"""
    return 256 // np.dtype(loop).itemsize


def lds_bytes(m, esz):
    blocks = -(-m // 16)
    w_pitch = blocks * 16 + (16 if blocks % 2 == 0 else 0)
    return (256 // esz * w_pitch + 64 * (256 // esz + 16 // esz)) * esz


# ------------------------------------------------------------------------------------------------------------ the chain, on the host
@functools.lru_cache(maxsize=1)
def _fma_program():
    if shutil.which("g++") is None:
        raise RuntimeError("tests/ml_fma.cpp needs g++")
    exe = os.path.join(tempfile.mkdtemp(prefix="ml_fma_"), "ml_fma")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tests", "ml_fma.cpp"), "-o", exe])
    return exe


def chain(x, w):
    """(rows, n) . (n, m) -> (rows, m): one fma chain per output in ascending k, in the arrays' type (float32 or float64)"""
    T = np.dtype(x.dtype)
    assert T == w.dtype and T in U and x.ndim == 2 and w.ndim == 2 and x.shape[1] == w.shape[0]
    d = os.path.dirname(_fma_program())
    fin, fout = os.path.join(d, f"in{os.getpid()}.bin"), os.path.join(d, f"out{os.getpid()}.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4i", int(T.itemsize == 8), x.shape[0], x.shape[1], w.shape[1]))
        f.write(np.ascontiguousarray(x).tobytes())
        f.write(np.ascontiguousarray(w).tobytes())
    subprocess.check_call([_fma_program(), fin, fout])
    out = np.fromfile(fout, dtype=T).reshape(x.shape[0], w.shape[1])
    os.remove(fin), os.remove(fout)
    return out


def activate(pre, act, typing="numba"):
    """the reference's activation of pre-activations in the loop's type; ``act`` a character"""
    T = pre.dtype.type
    f64 = np.float64
    with np.errstate(all="ignore"):
        if act == "r":
            return pre * (pre > 0).astype(T)
        if act == "l":
            if typing == "numpy2" or T is np.float64:
                return pre * (pre > 0).astype(T) + T(0.01) * pre * (pre < 0).astype(T)
            return ((pre * (pre > 0).astype(T)).astype(f64) + (0.01 * pre.astype(f64)) * (pre < 0).astype(f64)).astype(T)
        if act == "s":
            if typing == "numpy2" or T is np.float64:
                return T(1) / (T(1) + np.exp(-pre))
            return (1.0 / (1.0 + np.exp(-pre).astype(f64))).astype(T)
        if act == "m":
            if typing == "numpy2" or T is np.float64:
                return np.log(T(1) + np.exp(pre))
            return np.log(1.0 + np.exp(pre).astype(f64)).astype(T)
        if act == "t":
            return np.tanh(pre)
    return np.full(pre.shape, np.nan, dtype=T)


def normalise(x, means, variances):
    with np.errstate(all="ignore"):
        return ((x - means) / np.sqrt(variances)).astype(x.dtype)


def emulate(x, w, bias, act, means=None, variances=None, typing="numba"):
    """the device's result for rows x (any row type), weights w (n, m) or (n,), bias (m,) / a number / None, in the loop of x's type"""
    T = np.float64 if x.dtype == np.float64 else np.float32
    x = np.atleast_2d(x).astype(T)
    if means is not None:
        x = normalise(x, means.astype(T), variances.astype(T))
    w2 = w.astype(T).reshape(x.shape[1], -1)
    pre = chain(x, w2)
    if bias is not None:
        with np.errstate(all="ignore"):
            pre = (pre + np.asarray(bias, dtype=T).reshape(1, -1)).astype(T)
    out = activate(pre, act, typing)
    return out[:, 0] if w.ndim == 1 else out


# ------------------------------------------------------------------------------------------------------------ the exact evaluation and the bound
def _wide(T):
    return np.longdouble if np.dtype(T) == np.float64 else np.float64


def exact(x, w, bias, act, means=None, variances=None):
    """the reference body evaluated one precision up (float64 for the float32 loop, long double for the float64 loop) -> (value, magnitude):
    magnitude = sum_i |x_i w_ij| + |b_j|, what the dot product's bound scales with.  The normalisation, where given, is the loop's own
    (its result is the layer's input)."""
    T = np.float64 if x.dtype == np.float64 else np.float32
    W = _wide(T)
    x = np.atleast_2d(x).astype(T)
    if means is not None:
        x = normalise(x, means.astype(T), variances.astype(T))
    xw, ww = x.astype(W), w.astype(T).reshape(x.shape[1], -1).astype(W)
    with np.errstate(all="ignore"):
        pre = xw @ ww
        mag = np.abs(xw) @ np.abs(ww)
        if bias is not None:
            b = np.asarray(bias, dtype=T).astype(W).reshape(1, -1)
            pre, mag = pre + b, mag + np.abs(b)
        one = W(1)
        val = {"r": lambda p: p * (p > 0), "l": lambda p: p * (p > 0) + W(0.01) * p * (p < 0), "s": lambda p: one / (one + np.exp(-p)),
               "m": lambda p: np.log(one + np.exp(p)), "t": np.tanh}[act](pre)
    return (val[:, 0], mag[:, 0]) if w.ndim == 1 else (val, mag)


def ulp(v, T):
    """the spacing of type T at |v| (never below the smallest normal's)"""
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), float(np.finfo(T).tiny))
    return np.exp2(np.floor(np.log2(a)) - (np.finfo(T).nmant))


def bound(n, act, mag, val, T):
    return LIPSCHITZ[act] * (n + 2) * U[np.dtype(T)] * np.asarray(mag, dtype=np.float64) + act_ulps(T, act) * ulp(val, T)


def within(got, x, w, bias, act, means=None, variances=None):
    """-> (ok, worst ratio |got - exact| / bound) over the finite values; non-finite ones must agree in kind"""
    T = got.dtype.type
    val, mag = exact(x, w, bias, act, means, variances)
    val64 = np.asarray(val, dtype=np.float64)
    fin = np.isfinite(val64) & np.isfinite(np.asarray(mag, dtype=np.float64))
    kind_ok = np.array_equal(np.isnan(got[~fin]), np.isnan(val64[~fin])) and np.array_equal(got[~fin][~np.isnan(got[~fin])], val64[~fin][~np.isnan(val64[~fin])])
    n = np.atleast_2d(x).shape[1]
    err = np.abs(np.asarray(got.astype(_wide(T)) - val, dtype=np.float64))[fin]
    ratio = err / bound(n, act, mag, val, T)[fin]
    worst = float(ratio.max()) if ratio.size else 0.0
    return bool(kind_ok and np.isfinite(got[fin]).all() and worst <= 1.0), worst


# ------------------------------------------------------------------------------------------------------------ the book
def axes(rows):
    """the lengths, widths and row counts the kernel takes another path at: a k-step of 4, the chunk, a column block of 16, the 16 rows of a
    wavefront and the 64 of a workgroup"""
    c = chunk(LOOPS[rows])
    return (1, 3, 4, 5, c - 1, c, c + 1, 2 * c + 1), (1, 15, 16, 17, 33, M_MAX), (1, 15, 16, 17, 63, 64, 65, 130)


def shapes(rows):
    """(n, m, row count): every n with every m, the row counts taken in turn"""
    ns, ms, rs = axes(rows)
    return [(n, m, rs[(i * len(ms) + j) % len(rs)]) for i, n in enumerate(ns) for j, m in enumerate(ms)]


def _seed(*key):
    return abs(hash(tuple(int(k) for k in key))) % (2 ** 31)


KIND_ID = {"f32": 1, "i16": 2, "u16": 3, "f64": 4}


@functools.lru_cache(maxsize=None)
def rows_of(rows, count, n):
    rng = np.random.default_rng(_seed(KIND_ID[rows], count, n))
    if rows == "i16":
        return rng.integers(-2000, 2001, (count, n)).astype(np.int16)
    if rows == "u16":
        return rng.integers(0, 4001, (count, n)).astype(np.uint16)
    return rng.normal(0.0, 1.0, (count, n)).astype(ROWS[rows])


@functools.lru_cache(maxsize=None)
def layer_of(rows, n, m):
    """weights (n, m), bias (m,), means (n,), variances (n,) of the loop's type; pre-activations of order 1"""
    T = LOOPS[rows]
    rng = np.random.default_rng(_seed(KIND_ID[rows], n, m, 7))
    scale = (2000.0 if rows in ("i16", "u16") else 1.0) * np.sqrt(n)
    return ((rng.normal(0.0, 1.5, (n, m)) / scale).astype(T), rng.normal(0.0, 0.5, m).astype(T), rng.normal(0.0, 0.3, n).astype(T),
            rng.uniform(0.5, 2.0, n).astype(T))


def variant(k):
    """what case k of a list runs with: (activation, bias?)"""
    return ACTIVATIONS[k % 5], k % 2 == 0


@functools.lru_cache(maxsize=None)
def want(rows, n, m, count, act, with_bias, normalised=False, classify=False):
    x = rows_of(rows, count, n)
    w, b, mu, var = layer_of(rows, n, m)
    if classify:
        w, b = w[:, 0], b[0]
    return emulate(x, w, b if with_bias else None, act, mu if normalised else None, var if normalised else None)


def activation_distances():
    """{loop: {activation: ulps}}: over the book's pre-activations, the largest distance between the activation under numba's typing with
    NumPy's own functions and its evaluation one precision up"""
    worst = {"f32": dict.fromkeys("srlmt", 0.0), "f64": dict.fromkeys("srlmt", 0.0)}
    for rows in ROWS:
        T = LOOPS[rows]
        W, loop = _wide(T), "f64" if T is np.float64 else "f32"
        for n, m, count in shapes(rows):
            w, b, _mu, _var = layer_of(rows, n, m)
            p = (chain(rows_of(rows, count, n).astype(T), w) + b).astype(T)
            pw, one = p.astype(W), W(1)
            with np.errstate(all="ignore"):
                ex = {"r": pw * (pw > 0), "l": pw * (pw > 0) + W(0.01) * pw * (pw < 0), "s": one / (one + np.exp(-pw)), "m": np.log(one + np.exp(pw)),
                      "t": np.tanh(pw)}
            for act in "smt":
                d = np.abs(np.asarray(activate(p, act).astype(W) - ex[act], dtype=np.float64)) / ulp(ex[act], T)
                worst[loop][act] = max(worst[loop][act], float(d.max()))
    return worst


# ------------------------------------------------------------------------------------------------------------ the fixture: integer-valued layers
FIXTURE_SHAPES = ((1, 1), (5, 17), (63, 16), (64, 33), (129, 15), (1024, 256))  # (n, m); |x| <= 1024, |w| <= 8: every partial sum below 2^24
FIXTURE_ROWS = 9


def fixture_layer(n, m):
    rng = np.random.default_rng(_seed(n, m, 11))
    return (rng.integers(-1024, 1025, (FIXTURE_ROWS, n)).astype(np.float64), rng.integers(-8, 9, (n, m)).astype(np.float64),
            rng.integers(-64, 65, m).astype(np.float64))


def fixture_norm(n):
    """means and variances of the fixture's normalisation_layer: integers, the variances 1 .. 7 (most square roots and quotients inexact)"""
    return np.arange(n, dtype=np.float64) - 3.0, 1.0 + np.arange(n) % 7


# ------------------------------------------------------------------------------------------------------------ programs for the planner
def program(n, m, act="r", bias=True, norm=False, classify=False, dense=True, rows=np.float32, loop=np.float32, offset=0, row_stride=None,
            out_stride=None, act_code=None):
    """LOAD, [NORMALISE,] [DENSE,] STORE / STORE_SCALAR as the entry points and the recipe compiler write them"""
    from dspeed_amd import _lib
    from dspeed_amd.chain import Program

    p = Program()
    s = p.add_slot(n)
    p.add_op(_lib.OP_LOAD, dst=s, io=p.add_io("in", _lib.IO_WF_IN, rows, n, offset, row_stride))
    if norm:
        im, iv = p.add_io("means", _lib.IO_TAPS, loop, n, 0, 0), p.add_io("variances", _lib.IO_TAPS, loop, n, 0, 0)
        p.add_op(_lib.OP_NORMALISE, dst=s, src=s, io=im, ip=(iv,))
    if not dense:
        p.add_op(_lib.OP_STORE, src=s, io=p.add_io("out", _lib.IO_WF_OUT, loop, n, 0, out_stride))
        return p
    iw = p.add_io("kernel", _lib.IO_TAPS, loop, n * m, 0, 0)
    ib = p.add_io("bias", _lib.IO_TAPS, loop, m, 0, 0) if bias else -1
    code = ord(act) if act_code is None else act_code
    if classify:
        r = p.add_sregs(1)
        p.add_op(_lib.OP_DENSE, dst=r, src=s, io=iw, ip=(code, ib, n, 0))
        p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io("out", _lib.IO_SCALAR_OUT, loop), ip=(r,))
    else:
        o = p.add_slot(m)
        p.add_op(_lib.OP_DENSE, dst=o, src=s, io=iw, ip=(code, ib, n, m))
        p.add_op(_lib.OP_STORE, src=o, io=p.add_io("out", _lib.IO_WF_OUT, loop, m, 0, out_stride))
    return p
