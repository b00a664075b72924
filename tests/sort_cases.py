"""The case book of ``sort`` (dsp_sort.hip), shared by the CPU and the GPU tests.  Not collected: a plain helper.

A *case* is rows of one length and type that go through one launch: ``Case.w`` (R, n) in the rows' own type, one row per family (the list
below, cycled to R rows).  The expected output is NumPy's: ``np.sort`` of the row in the loop's type, and a row of NaNs where the row holds
a NaN (reference processors/sort.py:36-42).  Nothing of the code under test is its own yardstick.

Every length comes with every row count of ROW_COUNTS -- four rows to a workgroup and the remainders -- and the rows of the four counts
together hold every family of the type at that length."""
import os
import re

import numpy as np

from dspeed_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "dsp_sort_kernel"
F32_MAX = 16384  # DSP_SORT_F32_MAX; the float64 loop: half
# the narrow / wide threshold: dsp_sort::NARROW_MAX of dsp_kernels.h, the longest padded row a wavefront sorts alone
T = int(re.search(r"constexpr int NARROW_MAX = (\d+);", open(os.path.join(ROOT, "dspeed_amd", "csrc", "dsp_kernels.h")).read()).group(1))
LENGTHS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, T - 1, T, T + 1, 4095, 4096, 4097, 8192, 16383, 16384]
ROW_COUNTS = (1, 4, 5, 7)
IN_PAD, OUT_PAD = 3, 5  # rows n + 3 apart on the way in, n + 5 on the way out, canaries between
LOOPS = {"f32": np.float32, "i16": np.float32, "u16": np.float32, "f64": np.float64}
ROWS = {"f32": np.float32, "i16": np.int16, "u16": np.uint16, "f64": np.float64}
LIMITS = "rows of up to 16384 samples in the float32 loop and 8192 in the float64 loop"


def limit(rows):
    return F32_MAX // 2 if rows == "f64" else F32_MAX


def padded(n):
    p = 8
    while p < n:
        p *= 2
    return p


# ---------------------------------------------------------------------------------------------------------------- the families
def _float_family(name, n, ft, rng):
    tiny = np.finfo(ft).smallest_subnormal
    u = rng.uniform(-1, 1, n)
    if name == "sorted":
        return np.arange(n, dtype=ft) - n // 2
    if name == "reversed":
        return (n - np.arange(n, dtype=ft)) * ft(0.5)
    if name == "equal":
        return np.full(n, ft(7.25))
    if name == "alternating":
        return np.where(np.arange(n) % 2 == 0, ft(5), ft(-3)).astype(ft)
    if name == "duplicates":
        return rng.integers(-4, 5, n).astype(ft)
    if name == "denormals":  # mixed sign, an eighth of the samples denormal
        w = (u * 1e3).astype(ft)
        d = rng.random(n) < 0.125
        w[d] = (rng.integers(-5, 6, d.sum()) * tiny).astype(ft)
        return w
    if name == "infinities":
        w = u.astype(ft)
        k = rng.random(n) < 0.2
        w[k] = np.where(rng.random(k.sum()) < 0.5, ft(np.inf), ft(-np.inf))
        return w
    if name == "zeros":
        w = u.astype(ft)
        k = rng.random(n) < 0.4
        w[k] = np.where(rng.random(k.sum()) < 0.5, ft(0.0), ft(-0.0))
        return w
    if name == "inf-ties":  # real +inf samples: at a length below its padded one they tie with the padding
        w = u.astype(ft)
        w[::3] = np.inf
        return w
    if name.startswith("nan-"):
        w = (u * 100).astype(ft)
        w[{"nan-first": 0, "nan-middle": n // 2, "nan-last": n - 1}[name]] = np.nan
        return w
    raise KeyError(name)


def _int_family(name, n, it, rng):
    lo, hi = np.iinfo(it).min, np.iinfo(it).max
    if name == "extremes":
        return rng.choice(np.array([lo, lo + 1, -1 if lo < 0 else 1, 0, hi - 1, hi], dtype=it), n)
    if name == "sorted":
        return np.linspace(lo, hi, n).astype(it)
    if name == "reversed":
        return np.linspace(hi, lo, n).astype(it)
    if name == "equal":
        return np.full(n, hi, dtype=it)
    if name == "alternating":
        return np.where(np.arange(n) % 2 == 0, hi, lo).astype(it)
    if name == "duplicates":
        return rng.integers(0, 9, n).astype(it)
    if name == "baseline":
        return (10000 + rng.integers(-20, 21, n)).astype(it)
    raise KeyError(name)


# a clean row stands between any two NaN rows
FLOAT_FAMILIES = ("sorted", "nan-first", "reversed", "equal", "nan-middle", "alternating", "duplicates", "nan-last", "denormals", "infinities",
                  "zeros", "inf-ties", "denormals", "nan-middle", "zeros", "infinities", "duplicates")
INT_FAMILIES = ("extremes", "sorted", "reversed", "equal", "alternating", "duplicates", "baseline", "extremes", "baseline", "duplicates",
                "extremes", "sorted", "reversed", "alternating", "baseline", "extremes", "equal")
assert len(FLOAT_FAMILIES) == len(INT_FAMILIES) == sum(ROW_COUNTS)


class Case:
    def __init__(self, rows, n, first, count):
        self.rows, self.n, self.count = rows, n, count
        self.loop = LOOPS[rows]
        self.name = f"{rows}_n{n}_r{count}"
        fams = (FLOAT_FAMILIES if rows in ("f32", "f64") else INT_FAMILIES)[first:first + count]
        self.families = fams
        rng = np.random.default_rng([n, first, sorted(ROWS).index(rows)])
        make = _float_family if rows in ("f32", "f64") else _int_family
        self.w = np.stack([make(f, n, ROWS[rows], rng) for f in fams])
        assert self.w.dtype == ROWS[rows] and self.w.shape == (count, n)

    def want(self):
        """NumPy's answer in the loop's type: np.sort of a row, NaNs for a row that holds one"""
        x = self.w.astype(self.loop)
        out = np.sort(x, axis=1)
        out[np.isnan(x).any(axis=1)] = np.nan
        return out

    def nan_rows(self):
        return np.isnan(self.w.astype(self.loop)).any(axis=1)

    def strided_input(self, poison):
        """the rows n + IN_PAD apart in one block, `poison` between them"""
        block = np.full((self.count, self.n + IN_PAD), poison, dtype=self.w.dtype)
        block[:, :self.n] = self.w
        return block


def cases(rows):
    """every case of a type: for each length the four row counts, which share out the 17 family rows"""
    out = []
    for n in LENGTHS:
        if n > limit(rows):
            continue
        first = 0
        for count in ROW_COUNTS:
            out.append(Case(rows, n, first, count))
            first += count
    return out


def check(case, got, what):
    """value equality with NumPy, the multiset of bit patterns, the NaN rule"""
    want, nan = case.want(), case.nan_rows()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, case.name)
    assert np.array_equal(got, want, equal_nan=True), (what, case.name, [case.families[r] for r in np.flatnonzero((got != want).any(axis=1) & ~nan)])
    assert np.isnan(got[nan]).all() and not np.isnan(got[~nan]).any(), (what, case.name)
    # nothing lost, nothing duplicated: the output's bits, sorted as unsigned integers, are the input's (denormals, both zeros)
    ut = np.uint32 if case.loop is np.float32 else np.uint64
    x = case.w.astype(case.loop)
    assert np.array_equal(np.sort(got[~nan].view(ut), axis=1), np.sort(x[~nan].view(ut), axis=1)), (what, case.name)
    # -0.0 before +0.0: the total order of the bit patterns
    clean = got[~nan]
    assert not ((clean[:, 1:] == clean[:, :-1]) & np.signbit(clean[:, 1:]) & ~np.signbit(clean[:, :-1])).any(), (what, case.name)


# ---------------------------------------------------------------------------------------------------------------- the program
def program(n, rows=np.float32, loop=np.float32, offset=0, row_stride=None, out_len=None, out_stride=None):
    """LOAD, SORT, STORE"""
    from dspeed_amd.chain import Program

    p = Program()
    m = n if out_len is None else out_len
    s_in, s_out = p.add_slot(n), p.add_slot(m)
    p.add_op(_lib.OP_LOAD, dst=s_in, io=p.add_io("w", _lib.IO_WF_IN, rows, n, offset, row_stride))
    p.add_op(_lib.OP_SORT, dst=s_out, src=s_in)
    p.add_op(_lib.OP_STORE, src=s_out, io=p.add_io("out", _lib.IO_WF_OUT, loop, m, 0, out_stride))
    return p
