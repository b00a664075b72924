"""The case book of the waveform aligner -- inl_correction, get_wf_centroid, wf_alignment, wf_correction and the generator step -- and a NumPy
emulation of every rule the device follows (dsp_align.hip), the rows the reference leaves undefined included.  Plain helper, not collected.

The rules (reference processors/inl_correction.py, get_wf_centroid.py, wf_alignment.py, wf_correction.py, kernels.py:103-142), with numba's
typing -- which is NumPy 2's here -- written out:

  inl_correction   w_out[i] = T(float64(w_in[i]) + float64(inl[w_in[i]])): one rounding.  A NaN anywhere in inl: NaN rows, no range error.  A
                   sample outside [0, p): DSPFatal "ADC code {code} out of range for INL array of length {p}", the first such sample's.
  get_wf_centroid  lo, hi = first argmin, first argmax; a = first index of [lo, hi) with a sample > 0, b = last with a sample < 0;
                   centroid = T(round(((a + shift) + (b + shift)) / 2)) in float64, half to even.  A row with a NaN: NaN.
                   UNDEFINED in the reference (IndexError under CPython, a read out of bounds compiled): hi <= lo, no such a, no such b.
                   The device: NaN, no error.
  wf_alignment     float64 arithmetic, int() truncating; c, sh, s = centroid, shift, size:
                     1  c >= s/2 and c < n - s/2:       w_out = w_in[int(c - s/2) : int(c + s/2)]          (always s samples)
                     2  c > s/2 - sh and c < s/2:       ss = int((s + 1)/2 - c), k = int(c + s/2);  w_out[:ss] = w_in[0];  w_out[ss:] = w_in[:k]
                     3  otherwise:                      w_out = w_in[:s]
                   A row with a NaN: a NaN row.  A NaN centroid on a row without one: DSPFatal "centroid is nan".
                   UNDEFINED in the reference (ValueError in NumPy's broadcast): branch 2 where len(w_out[ss:]) != len(w_in[:k]) by Python's
                   slice rules and len(w_in[:k]) != 1 (one sample broadcasts).  The device: a NaN row, no error.
                   The two typings differ in one place: numba truncates a float slice bound (w_in[:size]), CPython refuses it (TypeError).  The
                   fixture's generator hands size to the body as a Python int; ``emulate_alignment(..., typing="cpython")`` refuses a float.
  wf_correction    a NaN in the row or anywhere in w_corr: a NaN row; else w_out = w_in with w_in[i] - w_corr[i - start] on [start, stop): one
                   subtraction in the loop's type.
  step             kernel[i] = 1 for len/4 <= i < 3 len/4 (comparisons of real numbers), else -1; weight_pos is not used.
"""
import numpy as np

from dspeed_amd import _lib

BOOK = "align"
KERNEL = "dsp_align_kernel"
LOOPS = {"f32": np.float32, "f64": np.float64}
OK, NUMPY_ERROR, FATAL = 0, 1, 2  # what the reference did with a row: returned, raised in NumPy (undefined), raised DSPFatal

LENGTHS = (2, 3, 63, 64, 65, 127, 128, 129, 1000, 4096)  # both sides of a wavefront's 64 lanes and of the loaders' groups, the shortest rows
ROW_COUNTS = (1, 2, 5, 67)  # partial workgroups of four rows


# ---------------------------------------------------------------------------------------------------------------- get_wf_centroid
def bipolar(n, lo, hi, last_neg, first_pos, T):
    """a row with its minimum at lo, its maximum at hi, negative up to last_neg, zero up to first_pos (exclusive), positive from there"""
    w = np.zeros(n, T)
    w[lo:last_neg + 1] = -1 - np.arange(last_neg + 1 - lo)[::-1] % 7
    w[lo] = -50
    w[first_pos:hi + 1] = 1 + np.arange(hi + 1 - first_pos) % 5
    w[hi] = 60
    return w


def centroid_rows(loop, n):
    """(names, rows of n samples): every pattern of the issue that fits n samples; ``defined`` is the emulation's to tell"""
    T = LOOPS[loop]
    names, rows = [], []

    def add(name, w):
        names.append(name)
        rows.append(np.asarray(w, T))

    add("constant", np.full(n, 3, T))
    add("inverted", np.where(np.arange(n) == 0, 9, np.where(np.arange(n) == n - 1, -9, 0)))
    add("adjacent", np.where(np.arange(n) == 0, -9, np.where(np.arange(n) == 1, 9, 0)))  # hi = lo + 1: nothing positive in [lo, hi)
    for at, name in ((0, "ramp-nan-first"), (n - 1, "ramp-nan-last")):
        v = np.arange(n) - (n // 2 - 0.5)
        v[at] = np.nan
        add(name, v)
    if n >= 3:
        add("ramp", np.arange(n) - (n // 2 - 0.5))  # lo = 0, hi = n - 1, the crossing in the middle
    if n >= 5:
        add("ramp-through-zero", np.arange(n) - n // 2)
        add("ramp-steep", 3 * (np.arange(n) - (n // 3 + 0.5)))
    if n >= 40:
        add("rising-positive", 1 + np.arange(n))
        add("step", np.where(np.arange(n) < n // 2, -2, 2))  # hi = the first of the equal maxima: the first sample behind the negatives
        for k, (lo, hi, ln, fp) in enumerate(((0, n - 1, 1, n - 2), (1, 38, 1, 37), (7, 33, 20, 21), (7, 33, 19, 22), (30, 39, 33, 36), (2, 9, 4, 5), (0, 2, 0, 1), (10, 20, 10, 19),
                                              (5, 35, 6, 7), (5, 35, 33, 34))):
            add(f"bipolar-{k}", bipolar(n, lo, hi, ln, fp, T))
    if n >= 40:
        add("measured", bipolar(n, 12, 26, 18, 20, T))  # the issue's row: 19, 22, 22 for shifts 0, 3, 2.5
        add("odd-18.5", bipolar(n, 12, 26, 18, 19, T))  # sums of both parities: a tie goes to the even number
        add("odd-19.5", bipolar(n, 12, 26, 19, 20, T))
        add("wide-gap", bipolar(n, 3, n - 2, 9, n - 5, T))
        add("no-negative-between", np.where(np.arange(n) == 5, -9, np.where(np.arange(n) == n - 3, 9, 1)))
        w = bipolar(n, 12, 26, 18, 20, T)
        for at, name in ((0, "nan-first"), (n - 1, "nan-last"), (11, "nan-before-lo"), (27, "nan-after-hi")):
            v = w.copy()
            v[at] = np.nan
            add(name, v)
        v = w.copy()
        v[30] = np.inf
        v[5] = -np.inf  # the extremes move to the infinities: lo = 5, hi = 30
        add("infinities", v)
    if n >= 129:
        add("lane-edge", bipolar(n, 63, 64 + 63, 64, 65, T))
        add("group-edge", bipolar(n, 64, 128, 70, 127, T))
        w = bipolar(n, 20, 100, 40, 60, T)
        w[70], w[110] = w[20], w[100]  # equal extremes in other lanes: the first of each wins (70 lies inside [lo, hi): negative there)
        add("ties", w)
    if n >= 1000:
        w = bipolar(n, 100, 700, 300, 500, T)
        w[900], w[950] = w[100], w[700]  # equal extremes in other groups of the loader
        add("ties-far", w)
        add("group-edges-far", bipolar(n, 255, 768, 256, 767, T))
        w = np.zeros(n, T)
        w[:512], w[512:] = -1, 1  # every sample an extreme: lo = 0, hi = 512
        add("all-ties", w)
    return names, np.stack(rows)


def centroid_shifts(n):
    """shifts valid for rows of n samples: none, a whole number, a half (non-integral: the tie rule), the largest"""
    return tuple(s for s in (0.0, 3.0, 2.5, float(n - 1)) if s <= n - 1)


def emulate_centroid(rows, shift, T):
    """-> (centroids of type T, NaN where the device gives NaN; ``defined``: False where the reference defines no result)"""
    rows = np.atleast_2d(rows)
    out, defined = np.full(len(rows), np.nan, T), np.ones(len(rows), bool)
    sh = np.float64(T(shift))
    for r, w in enumerate(rows):
        if np.isnan(w).any():
            continue
        lo, hi = int(np.argmin(w)), int(np.argmax(w))
        between = w[lo:hi] if hi > lo else w[:0]
        pos, neg = np.flatnonzero(between > 0), np.flatnonzero(between < 0)
        if not (pos.size and neg.size):
            defined[r] = False
            continue
        c_a, c_b = np.float64(lo + pos[0]) + sh, np.float64(lo + neg[-1]) + sh
        out[r] = T(np.rint((c_a + c_b) / 2))
    return out, defined


# ---------------------------------------------------------------------------------------------------------------- wf_alignment
def align_rows(loop, n, rows_dtype=None):
    """(names, rows): distinct samples, so that every sample of a window says where it came from; float rows also with NaNs"""
    T = LOOPS[loop] if rows_dtype is None else rows_dtype
    base = (100 + 3 * np.arange(n) + (np.arange(n) % 5)).astype(T)
    names, rows = ["ramp", "ramp-2"], [base, (base[::-1] - 50).astype(T)]
    if np.dtype(T).kind == "f":
        for at, name in ((0, "nan-first"), (n - 1, "nan-last"), (n // 2, "nan-middle")):
            v = base.copy()
            v[at] = np.nan
            names.append(name)
            rows.append(v)
    return names, np.stack(rows)


def align_params(n):
    """(centroid, shift, size) for rows of n samples: each branch at both of its edges, odd and even sizes, size 1 and n, negative and
    non-integral centroids, the broadcasts NumPy allows and those it refuses"""
    out = []
    for s in sorted({1, 2, 9, 10, 63, 64, 65, n} & set(range(1, n + 1))):
        h = s / 2
        for sh in sorted({0.0, 2.0, float(min(8, n)), float(n)}):
            cs = {h, h - 1, h - 0.5, n - h - 1, n - h, n - h + 1, h - sh, h - sh + 1, h - sh + 0.5, float(n), 0.0, -1.0, -h, -h + 1, 1 - h, 2 - h, 3.7, -3.4, -3.7,
                  5.5, h + 0.25, np.inf, -np.inf}
            out += [(float(c), sh, s) for c in sorted(cs)]
    return out


def align_window(c, sh, s, n):
    """-> ("window", first) | ("pad", fill, count) | ("head",) | None where the reference fails in NumPy's broadcast"""
    c, sh, half = np.float64(c), np.float64(sh), s / 2
    if c >= half and c < n - half:
        return ("window", int(c - half))
    if c > half - sh and c < half:
        ss, k = int((s + 1) / 2 - c), int(c + half)
        lhs, rhs = len(range(s)[ss:]), len(range(n)[:k])  # Python's slice rules
        if lhs != rhs and rhs != 1:
            return None
        return ("pad", s - lhs, rhs)
    return ("head",)


def emulate_alignment(rows, centroid, shift, size, T, typing="numba"):
    """-> (windows of type T, status per row: OK, NUMPY_ERROR -- a NaN row on the device --, FATAL -- "centroid is nan").  ``centroid``: one value
    or a value per row.  ``rows`` may be integers: they hold no NaN."""
    if typing == "cpython" and not isinstance(size, (int, np.integer)):
        raise TypeError("slice indices must be integers or None or have an __index__ method")
    rows = np.atleast_2d(rows)
    s, n = int(size), rows.shape[1]
    cs = np.broadcast_to(np.asarray(centroid, T), (len(rows),))
    out, status = np.full((len(rows), s), np.nan, T), np.zeros(len(rows), np.int8)
    for r, w in enumerate(rows):
        if w.dtype.kind == "f" and np.isnan(w).any():
            continue
        if np.isnan(cs[r]):
            status[r] = FATAL
            continue
        win = align_window(cs[r], T(shift), s, n)
        if win is None:
            status[r] = NUMPY_ERROR
        elif win[0] == "window":
            out[r] = w[win[1]:win[1] + s]
        elif win[0] == "head":
            out[r] = w[:s]
        else:
            out[r, :win[1]] = w[0]
            out[r, win[1]:] = w[:win[2]] if win[2] != 1 else w[0]
    return out, status


# ---------------------------------------------------------------------------------------------------------------- wf_correction
def correction_rows(loop, n):
    T = LOOPS[loop]
    base = (1000 + 7 * np.arange(n) % 113 + 0.25 * (np.arange(n) % 3)).astype(T)
    names, rows = ["plain", "infinite"], [base, np.where(np.arange(n) == n // 3, np.inf, base).astype(T)]
    for at, name in ((0, "nan-first"), (n - 1, "nan-last")):
        v = base.copy()
        v[at] = np.nan
        names.append(name)
        rows.append(v)
    return names, np.stack(rows)


def template(loop, m, nan_at=None):
    t = (0.1 + 0.37 * np.arange(m) + (np.arange(m) % 4) * 1e-3).astype(LOOPS[loop])
    if nan_at is not None:
        t[nan_at] = np.nan
    return t


def correction_params(n):
    """(m, start, stop, index of a NaN in the template or None): accepted by the reference's checks"""
    out = {(n, 0, n, None), (max(n // 2, 1), 0, 1, None), (1, n - 1, n, None), (n + 3, 0, n, None), (max(n - 1, 1), 0, max(n - 1, 1), None)}
    if n >= 129:
        out |= {(40, 50, 80, None), (40, 50, 90, None), (200, 63, 129, None), (40, 50, 80, 39), (40, 50, 80, 0)}  # (a window across a 64-sample edge; a NaN outside the part used)
    return sorted(out, key=lambda p: tuple(-1 if x is None else x for x in p))


CORRECTION_REFUSALS = [  # (n, m, start, stop, text)
    (129, 40, -1, 10, "start_idx must be positive"), (129, 40, 130, 140, "start_idx must be shorter than input waveform size"), (129, 40, 0, 0, "stop_idx must be positive"),
    (129, 40, 0, 130, "stop_idx must be shorter than input waveform size"), (129, 40, 10, 10, "start_idx must be smaller than stop_idx"),
    (129, 40, 20, 10, "start_idx must be smaller than stop_idx"), (129, 40, 50, 91, "stop_idx - start_idx must be smaller than len\\(w_corr\\)")]


def emulate_correction(rows, w_corr, start, stop, T):
    rows = np.atleast_2d(rows).astype(T)
    out = np.full(rows.shape, np.nan, T)
    if np.isnan(w_corr).any():
        return out
    for r, w in enumerate(rows):
        if np.isnan(w).any():
            continue
        out[r] = w
        out[r, start:stop] = w[start:stop] - np.asarray(w_corr, T)[:stop - start]
    return out


# ---------------------------------------------------------------------------------------------------------------- inl_correction
INL_BIG = (1 << 24) + 64  # a table long enough for codes above 2**24, where a float32 sum and the float64 sum rounded once part


def inl_table(loop, p, nan_at=None):
    T = LOOPS[loop]
    if p == INL_BIG:
        t = np.zeros(p, T)
        t[(1 << 24) + np.arange(64)] = 0.5 + 0.25 * (np.arange(64) % 3)  # fractional entries where the codes are odd and even
    else:
        t = ((np.arange(p) % 17 - 8) * 0.125 + (np.arange(p) % 3) * 0.01).astype(T)
    if nan_at is not None:
        t[nan_at] = np.nan
    return t


def inl_cases(loop):
    """(name, rows of integers, p, index of a NaN in the table or None): codes 0 and p - 1, every row type, the three table lengths, a row
    with the code p or a negative code among several (DSPFatal, or NaN rows under a table with a NaN), int32 codes above 2**24"""
    n = 130
    i = np.arange(3 * n).reshape(3, n)
    out = [("p1", np.zeros((2, 5), np.uint16), 1, None),
           ("p256-u16", (i * 7 % 256).astype(np.uint16), 256, None),
           ("p256-i16", np.where(i % 50 == 0, 255, np.where(i % 50 == 1, 0, i * 11 % 256)).astype(np.int16), 256, None),
           ("p65536-u16", np.where(i % 40 == 0, 65535, (i * 523) % 65536).astype(np.uint16), 65536, None),
           ("p65536-i32", ((i * 1237) % 65536).astype(np.int32), 65536, None),
           ("p65536-u32", ((i * 777) % 65536).astype(np.uint32), 65536, None),
           ("nan-table", (i * 7 % 256).astype(np.uint16), 256, 200),
           ("big-i32", ((1 << 24) + (i % 64)).astype(np.int32), INL_BIG, None)]
    over = (i * 7 % 256).astype(np.int32)
    over[1, 77], over[1, 100] = 256, 300  # the first offending sample is named
    out.append(("code-p", over, 256, None))
    under = (i * 7 % 256).astype(np.int16)
    under[2, 3] = -4
    out.append(("code-negative", under, 256, None))
    out.append(("nan-table-code-p", over, 256, 0))  # the reference returns first: NaN rows, no error
    return out


def emulate_inl(rows, table, T):
    """-> (rows of type T, status per row, text of the first DSPFatal or None)"""
    rows = np.atleast_2d(rows)
    out, status, text = np.full(rows.shape, np.nan, T), np.zeros(len(rows), np.int8), None
    if np.isnan(table).any():
        return out, status, text
    p = len(table)
    for r, w in enumerate(rows):
        codes = w.astype(np.int64)
        bad = np.flatnonzero((codes < 0) | (codes >= p))
        if bad.size:
            status[r] = FATAL
            text = text or f"ADC code {codes[bad[0]]} out of range for INL array of length {p}"
            continue
        out[r] = (codes.astype(np.float64) + table[codes].astype(np.float64)).astype(T)
    return out, status, text


# ---------------------------------------------------------------------------------------------------------------- step
def emulate_step(n, T=np.float32):
    return np.array([1 if n / 4 <= i < 3 * n / 4 else -1 for i in range(n)], T)


def tile_rows(a, count):
    """``count`` rows (or values) that repeat those of ``a`` in turn"""
    a = np.asarray(a)
    return a[np.arange(count) % len(a)]


# ---------------------------------------------------------------------------------------------------------------- programs
def program(n, op="inl", rows=None, loop=np.float32, size=10, centroid=5.0, shift=0.0, start=0, stop=1, table_len=None, table_dtype=None, store_aligned=True,
            offset=0, row_stride=None, out_stride=None, out_len=None, size_arg=None):
    """LOAD, then by ``op``: "inl" INL_CORRECTION, STORE | "centroid" WF_CENTROID, STORE_SCALAR | "align" WF_ALIGNMENT, STORE | "correct"
    WF_CORRECTION, STORE | "fused" WF_ALIGNMENT, WF_CORRECTION, [STORE of the aligned row,] STORE.  ``centroid``: a value, or "column"."""
    from dspeed_amd.chain import Program, Scalar

    if rows is None:
        rows = np.uint16 if op == "inl" else loop
    p = Program()
    s_in = p.add_slot(n)
    p.add_op(_lib.OP_LOAD, dst=s_in, io=p.add_io("w", _lib.IO_WF_IN, rows, n, offset, row_stride))

    def table(name, default):
        return p.add_io(name, _lib.IO_TAPS, loop if table_dtype is None else table_dtype, default if table_len is None else table_len, 0, 0)

    def store(slot, name):
        p.add_op(_lib.OP_STORE, src=slot, io=p.add_io(name, _lib.IO_WF_OUT, loop, p.slots[slot], 0, out_stride))

    if op == "inl":
        s_out = p.add_slot(n if out_len is None else out_len)
        p.add_op(_lib.OP_INL_CORRECTION, dst=s_out, src=s_in, io=table("inl", 256))
        store(s_out, "out")
    elif op == "centroid":
        reg = p.add_sregs(1)
        p.add_op(_lib.OP_WF_CENTROID, dst=reg, src=s_in, sp=(Scalar.const(shift),))
        p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io("centroid", _lib.IO_SCALAR_OUT, loop), ip=(reg,))
    elif op in ("align", "fused"):
        s_al = p.add_slot(size if out_len is None else out_len)
        c = Scalar.input(p.add_io("c", _lib.IO_SCALAR_IN, loop)) if isinstance(centroid, str) else Scalar.const(centroid)
        p.add_op(_lib.OP_WF_ALIGNMENT, dst=s_al, src=s_in, sp=(c, Scalar.const(shift), Scalar.const(size if size_arg is None else size_arg)))
        if op == "fused":
            s_out = p.add_slot(p.slots[s_al])
            p.add_op(_lib.OP_WF_CORRECTION, dst=s_out, src=s_al, io=table("w_corr", size), ip=(start, stop))
            if store_aligned:
                store(s_al, "aligned")
            store(s_out, "out")
        else:
            store(s_al, "out")
    else:
        s_out = p.add_slot(n if out_len is None else out_len)
        p.add_op(_lib.OP_WF_CORRECTION, dst=s_out, src=s_in, io=table("w_corr", n), ip=(start, stop))
        store(s_out, "out")
    return p
