"""Cases of histogram and histogram_stats (dsp_hist.hip): the rows tools/gen_golden_histogram.py feeds to the reference's bodies
(tests/golden/histogram.npz holds them with the expectations), the two rule sets of the float32 loop spelled out, and a NumPy model of the
kernel's formulation -- groups of 64 N samples, N per lane; the skip of the maximum; the drop of k >= m; histogram_stats as rounds of 64
bins and ballots -- that test_histogram_cases_cpu.py holds against the fixtures before anything runs on a GPU.  Nothing here needs a GPU
or the reference.  Every row comes from a seed.

What pins what:
  float64 loop    the reference's body as written (NumPy and numba agree on it).
  float32 loop    numba types ``float32 / int64`` as float64, so delta, np.linspace and the quotient are float64 while ``w - borders[0]`` and
                  ``max - min`` stay float32 (``numba_rules``); run under NumPy 2 the body keeps all of it in float32 (``numpy2_*`` in the
                  fixture, for the record).  The device follows ``numba_rules``; general float32 rows are pinned by that emulation only.
                  Rows marked exact -- integer-valued samples below 2^24 whose range is m * 2^j -- have exact borders, delta and quotients
                  under either rule set: there the body's own output is the expectation, and the emulation has to reproduce it.
  histogram_stats typing-independent (0.5 * w is exact, the rest float differences and comparisons): both loops pinned by the body.
"""
import numpy as np

BOOK = "histogram"
KERNEL = "histogram"
KERNEL_STATS = "histogram_stats"
MAX_BINS = 2048  # DSP_HIST_MAX_BINS
#: samples per lane the kernels are built with: 1 (unaligned rows), 2 (float64), 4 (float32), 8 (int16, uint16)
LANE_SAMPLES = (1, 2, 4, 8)
LENGTHS = (1, 3, 63, 64, 65, 255, 256, 257, 1000, 1024, 8192)
BINS = (1, 2, 63, 64, 65, 100, MAX_BINS)


def bins_for(n):
    """the numbers of bins a length is run with: every length meets 100 (the SiPM recipes'), every number of bins several lengths"""
    if n == 8192:
        return (100,)
    if n >= 1000:
        return BINS if n == 1024 else (1, 63, 100)
    if n >= 255:
        return (1, 64, 100)
    if n >= 63:
        return (2, 63, 65, 100)
    return (1, 2, 100)


# ------------------------------------------------------------------------------------------------------------------------------------
# rows
# ------------------------------------------------------------------------------------------------------------------------------------
def _general_rows(n, rng, short):
    """[(name, row as float64 values that are float32 numbers)]"""
    rows = [("spread", rng.uniform(-1000, 1000, n).astype(np.float32)),           # rows spread over the bins
            ("noise", (1000 + 5 * rng.standard_normal(n)).astype(np.float32)),     # concentrated in a few bins
            ("max_many", rng.integers(0, 8, n).astype(np.float32))]                # the maximum occurs many times
    if not short:
        rows += [("noise_int", np.rint(200 + 3 * rng.standard_normal(n)).astype(np.float32)),
                 ("two_valued", rng.integers(0, 2, n).astype(np.float32)),
                 ("constant", np.full(n, 3, dtype=np.float32))]
    if n >= 3:  # every sample but two in one bin: the minimum and the maximum stand alone
        w = np.full(n, 7, dtype=np.float32)
        w[int(rng.integers(0, n))] = 0
        free = [i for i in range(n) if w[i] == 7]
        w[free[int(rng.integers(0, len(free)))]] = 100
        rows.append(("contention", w))
    for name, at in (("nan_first", 0), ("nan_last", n - 1), ("nan_mid", n // 2)):
        if short and name != "nan_mid":
            continue
        w = rng.integers(-3, 4, n).astype(np.float32)
        w[at] = np.nan
        rows.append((name, w))
    return rows


def exact_rows(n, m, rng):
    """rows on which either rule set of the float32 loop computes the same: integers, range m * 2^j.  On the borders: every sample a border."""
    rows = []
    if n < 2:
        return rows
    for name, j, on in (("exact_on_borders", 0, True), ("exact_j2", 2, False))[n >= 4096:]:  # (the long rows: one exact row each)
        lo = int(rng.integers(-500, 500))
        step = 1 << j
        w = lo + (rng.integers(0, m + 1, n) * step if on else rng.integers(0, m * step + 1, n))
        a, b = rng.choice(n, 2, replace=False)
        w[a], w[b] = lo, lo + m * step
        assert np.abs(w).max() < 1 << 24
        rows.append((name, w.astype(np.float32)))
    return rows


class Group:
    """rows of one length and type that go through one launch per number of bins: ``w`` (R, n) general rows, ``x[m]`` the exact rows of m"""

    def __init__(self, name, tag, rows_dtype, n, names, w, ms, x):
        self.name, self.tag, self.rows_dtype, self.n, self.names, self.w, self.ms, self.x = name, tag, rows_dtype, n, names, w, ms, x
        self.loop = np.float32 if tag == "f32" else np.float64

    def rows(self, m):
        """the rows run with m bins, in the rows' own type: the general ones, then the exact ones"""
        return np.concatenate([self.w, self.x[m]]) if len(self.x[m]) else self.w

    def exact(self, m):
        return np.r_[np.zeros(len(self.w), bool), np.ones(len(self.x[m]), bool)]


def key(m, what):
    return f"m{m}_{what}"


def groups():
    out = []
    plan = [("f32", np.float32, LENGTHS), ("i16", np.int16, (257, 1000, 4096)), ("u16", np.uint16, (65, 1024)), ("f64", np.float64, (3, 257, 1000))]
    for pre, dt, lengths in plan:
        for n in lengths:
            rng = np.random.default_rng([0x4157, n, len(pre), ord(pre[0])])
            rows = _general_rows(n, rng, short=n >= 4096)
            if np.dtype(dt).kind in "iu":  # integer rows: the same families rounded into the type's range, no NaN
                rows = [(nm, np.rint(w) + (2000 if dt == np.uint16 else 0)) for nm, w in rows if not nm.startswith("nan")]
            if dt == np.float64:  # float64 rows are no float32 numbers
                rows = [(nm, w.astype(np.float64) * (1 + 2.0 ** -30) if nm in ("spread", "noise") else w.astype(np.float64)) for nm, w in rows]
            ms = bins_for(n) if pre == "f32" else (((64, 100) if n < 4096 else (100,)) if pre != "f64" else ((65, 100) if n == 1000 else bins_for(n)))
            x = {m: np.array([w for _, w in exact_rows(n, m, rng)]).reshape(-1, n).astype(dt if dt != np.uint16 else np.float64) for m in ms}
            if dt == np.uint16:
                x = {m: (v + 2000).astype(dt) for m, v in x.items()}
            tag = "f64" if dt == np.float64 else "f32"
            out.append(Group(f"{pre}_n{n}", tag, dt, n, [nm for nm, _ in rows], np.array([w for _, w in rows]).astype(dt), list(ms), x))
    return out


def stats_groups():
    """[(name, tag, m, weights (R, m), edges (R, m + 1), max_in (R,), row names)]: weights with ties and zeros around the mode, peaks in the
    first and last bin, NaN weights and NaN edges; max_in NaN, inside, on the middle between two edges, below edges[0], beyond edges[-2]"""
    out = []
    for tag, T in (("f32", np.float32), ("f64", np.float64)):
        for m in BINS if tag == "f32" else (1, 65, 100):
            rng = np.random.default_rng([0x57A7, m, len(tag), T(0).itemsize])
            i = np.arange(m)
            shapes = []
            for p in sorted({0, m - 1, int(rng.integers(0, m))} | ({m // 2, min(m - 1, 63), min(m - 1, 64)} if m < 1024 else set())):
                tri = np.maximum(0, 40 - 3 * np.abs(i - p))
                shapes.append((f"tri{p}", tri))
                holes = tri.copy()
                holes[(np.abs(i - p) > 0) & (np.abs(i - p) % 3 != 0)] = 0  # zeros around the mode: the searches step over empty bins
                shapes.append((f"holes{p}", holes))
                flat = tri.copy()
                flat[max(0, p - 2):p + 3] = tri.max()  # a plateau: the first of the largest weights
                shapes.append((f"plateau{p}", flat))
            shapes += [("zeros", np.zeros(m)), ("ints", rng.integers(0, 4, m)), ("ints_b", rng.integers(0, 30, m)), ("rising", i + 1.0), ("falling", m - i + 0.0),
                       ("negative", rng.integers(-5, 6, m))]
            lo, width = T(-3.25), T(0.37)
            edges = (lo + np.arange(m + 1).astype(T) * width).astype(T)
            names, W, E, M = [], [], [], []
            for nm, wts in shapes:
                picks = [("nan", np.nan), ("inside", edges[int(rng.integers(0, m))] + T(0.3) * width), ("below", edges[0] - T(1)),
                         ("beyond", edges[-2] + T(0.01)), ("past_end", edges[-1] + T(5))]
                if m > 1:
                    picks.append(("midway", (edges[0] + edges[1]) / T(2)))
                for pn, mi in picks if nm.startswith(("tri", "ints")) else picks[:1]:
                    names.append(f"{nm}_{pn}")
                    W.append(np.asarray(wts, dtype=T))
                    E.append(edges)
                    M.append(mi)
            for pn, mi in (("nan", np.nan), ("inside", 0.5)):
                names.append(f"nan_edges_{pn}")  # what histogram leaves for a row with a NaN
                W.append(np.zeros(m, dtype=T))
                E.append(np.full(m + 1, np.nan, dtype=T))
                M.append(mi)
                wn = np.asarray(shapes[0][1], dtype=T).copy()
                wn[m // 3] = np.nan
                names.append(f"nan_weight_{pn}")
                W.append(wn)
                E.append(edges)
                M.append(mi)
            out.append((f"stats_{tag}_m{m}", tag, m, np.array(W, dtype=T), np.array(E, dtype=T), np.array(M, dtype=T), names))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# the rule sets of the float32 loop, and the float64 loop, row by row
# ------------------------------------------------------------------------------------------------------------------------------------
def numba_rules(w, m, T):
    """(weights, borders, largest k) of one row in the loop's type T as numba types the body: float64 wherever an int64 meets a float"""
    w = np.asarray(w, dtype=T)
    weights, borders = np.zeros(m, dtype=T), np.full(m + 1, np.nan, dtype=T)
    if np.isnan(w).any():
        return weights, borders, -1
    lo, hi = w.min(), w.max()
    with np.errstate(over="ignore", invalid="ignore"):
        delta = np.float64(T(hi - lo)) / np.float64(m)
        borders[:] = (np.float64(lo) + np.arange(m + 1, dtype=np.float64) * delta).astype(T)
    borders[m] = hi
    if delta == 0:
        return weights, borders, -1
    rest = w[w != hi]
    k = np.floor((rest - borders[0]).astype(T).astype(np.float64) / delta).astype(np.int64)
    np.add.at(weights, k[k < m], 1)
    return weights, borders, int(k.max()) if len(k) else -1


# ------------------------------------------------------------------------------------------------------------------------------------
# the kernel's formulation
# ------------------------------------------------------------------------------------------------------------------------------------
def model_histogram(w, m, T, N):
    """dsp_hist_kernel on one row: samples dealt to (group, lane, j) as the loads deal them, both passes over the same positions"""
    w = np.asarray(w)
    n = len(w)
    per_group = 64 * N
    n_groups = -(-n // per_group)
    at = (np.arange(n_groups)[:, None, None] * per_group + np.arange(64)[None, :, None] * N + np.arange(N)[None, None, :]).reshape(-1)
    at = at[at < n]
    assert np.array_equal(np.sort(at), np.arange(n))  # every sample once
    x = w[at].astype(T)
    counters = np.zeros((m + 63) & ~63, dtype=np.uint32)
    bad = bool(np.isnan(x).any())
    lo, hi = (x.min(), x.max()) if not bad else (T(0), T(0))
    bad = bad or bool(np.isinf(lo) or np.isinf(hi))
    with np.errstate(over="ignore", invalid="ignore"):
        delta = np.float64(T(hi - lo)) / np.float64(m)
        if not bad and delta != 0:
            q = (x - lo).astype(T).astype(np.float64) / delta
            take = (x != hi) & (q < m)
            np.add.at(counters, q[take].astype(np.int64), 1)
        borders = (np.float64(lo) + np.arange(m + 1, dtype=np.float64) * delta).astype(T)
    borders[m] = hi
    if bad:
        borders[:] = np.nan
    return counters[:m].astype(T), borders


def _first_best(values, index, greater):
    """the exchange across the lanes: the better value, the lower index between equals; a NaN neither wins nor yields"""
    v, i = values[0], index[0]
    for ov, oi in zip(values[1:], index[1:]):
        if (ov > v if greater else ov < v) or (ov == v and oi < i):
            v, i = ov, oi
    return int(i)


def model_stats(weights, edges, max_in, T):
    """hist_stats: a bin per lane and round, per-lane first bests, ballots for the two searches"""
    wt, ed, max_in = np.asarray(weights, dtype=T), np.asarray(edges, dtype=T), T(max_in)
    m = len(wt)
    nan = T(np.nan)
    if np.isnan(wt).any():
        return nan, nan, nan
    with np.errstate(invalid="ignore"):
        def lanes(values, greater):
            bv, bi = np.full(64, values[0], dtype=T), np.zeros(64, dtype=np.int64)
            for i in range(m):
                lane = i % 64
                if (values[i] > bv[lane]) if greater else (values[i] < bv[lane]):
                    bv[lane], bi[lane] = values[i], i
            return _first_best(bv, bi, greater)

        if np.isnan(max_in):
            idx = lanes(wt, True)
        elif max_in > ed[m - 1]:
            idx = m - 1
        else:
            idx = lanes(np.abs((max_in - ed[:m]).astype(T)), False)
        edge, half = ed[idx], 0.5 * np.float64(wt[idx])
        fwhm = nan
        for base in range(idx & ~63, m, 64):
            i = np.arange(base, min(base + 64, m))
            hit = (i >= idx) & (wt[i].astype(np.float64) <= half) & (wt[i] != 0)
            if hit.any():
                fwhm = np.abs(T(edge - ed[i[hit][0]]))
                break
        for base in range(0, idx, 64):
            i = np.arange(base, min(base + 64, idx))
            hit = (wt[i].astype(np.float64) >= half) & (wt[i] != 0)
            if hit.any():
                other = np.abs(T(edge - ed[i[hit][0]]))
                fwhm = other if fwhm < other else fwhm
                break
    return T(idx), edge, T(fwhm)


# ------------------------------------------------------------------------------------------------------------------------------------
# rows whose bin index reaches m (no fixture holds one: the reference stores past the end of weights_out there)
# ------------------------------------------------------------------------------------------------------------------------------------
def dropping_rows(n, m, T, seed=0xD0):
    """(rows (6, n) of type T, expected weights (6, m), samples dropped per row).  Rows 1, 2 and 4 hold a minimum of -big, a maximum of 1, samples
    of -big / 2 (bin m / 2, exactly) and samples of 0.5 and 0.25: big is so large that 0.5 + big and 0.25 + big round to big = max - min in T,
    so their quotient is m exactly -- k = m, dropped.  m a power of two: delta = big / m is exact.  Rows 0, 3 and 5 are ordinary (integers
    0 .. m, range m: exact bins) and sit beside them in the same workgroups."""
    assert m & (m - 1) == 0 and m >= 2 and n >= 4
    big = T(1e8) if T is np.float32 else T(1e17)
    assert T(T(0.5) + big) == big and T(T(1) + big) == big
    rng = np.random.default_rng([seed, n, m])
    rows, want, dropped = np.zeros((6, n), dtype=T), np.zeros((6, m), dtype=T), np.zeros(6, dtype=np.int64)
    for r in range(6):
        if r in (1, 2, 4):
            kind = rng.integers(0, 3, n)  # 0: -big / 2, 1: 0.5, 2: 0.25
            row = np.where(kind == 0, -big / 2, np.where(kind == 1, T(0.5), T(0.25))).astype(T)
            a, b = rng.choice(n, 2, replace=False)
            row[a], row[b] = -big, 1
            kind[[a, b]] = -1
            want[r, 0], want[r, m // 2], dropped[r] = 1, (kind == 0).sum(), (kind > 0).sum()
        else:
            row = rng.integers(0, m + 1, n).astype(T)
            a, b = rng.choice(n, 2, replace=False)
            row[a], row[b] = 0, m
            want[r] = np.bincount(row[row != m].astype(np.int64), minlength=m)[:m]
        rows[r] = row
    assert dropped[[1, 2, 4]].min() > 0
    return rows, want, dropped


# ------------------------------------------------------------------------------------------------------------------------------------
# the programs the planner accepts (built with the package's own Program; nothing here touches a device)
# ------------------------------------------------------------------------------------------------------------------------------------
def hist_program(n, m, rows_dtype=np.float32, loop=np.float32, stats=False, stores=True, max_in=np.nan, borders_len=None, offset=0, row_stride=None,
                 max_blocks=0):
    """LOAD, HISTOGRAM[, HISTOGRAM_STATS][, STORE, STORE][, STORE_SCALAR x 3]; bindings wf, weights, borders, max_in (a column when
    ``max_in`` is "column"), mode, max, fwhm"""
    from dspeed_amd import _lib
    from dspeed_amd.chain import Program, Scalar

    p = Program()
    borders_len = m + 1 if borders_len is None else borders_len
    p.slots = [n, m, borders_len]
    p.n_sregs = 3 if stats else 0
    p.add_op(_lib.OP_LOAD, dst=0, io=p.add_io("wf", _lib.IO_WF_IN, rows_dtype, n, offset, row_stride))
    p.add_op(_lib.OP_HISTOGRAM, dst=1, src=0, ip=(2, max_blocks))
    if stats:
        mi = Scalar.input(p.add_io("max_in", _lib.IO_SCALAR_IN, loop)) if isinstance(max_in, str) else Scalar.const(max_in)
        p.add_op(_lib.OP_HISTOGRAM_STATS, src=1, ip=(2, 0), sp=(mi,))
    if stores:
        p.add_op(_lib.OP_STORE, src=1, io=p.add_io("weights", _lib.IO_WF_OUT, loop, m))
        p.add_op(_lib.OP_STORE, src=2, io=p.add_io("borders", _lib.IO_WF_OUT, loop, borders_len))
    if stats:
        for k, name in enumerate(("mode", "max", "fwhm")):
            p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io(name, _lib.IO_SCALAR_OUT, loop), ip=(k,))
    return p


def stats_program(m, loop=np.float32, max_in=np.nan, edges_len=None):
    """LOAD weights, LOAD edges, HISTOGRAM_STATS, STORE_SCALAR x 3"""
    from dspeed_amd import _lib
    from dspeed_amd.chain import Program, Scalar

    p = Program()
    edges_len = m + 1 if edges_len is None else edges_len
    p.slots = [m, edges_len]
    p.n_sregs = 3
    p.add_op(_lib.OP_LOAD, dst=0, io=p.add_io("weights", _lib.IO_WF_IN, loop, m))
    p.add_op(_lib.OP_LOAD, dst=1, io=p.add_io("edges", _lib.IO_WF_IN, loop, edges_len))
    mi = Scalar.input(p.add_io("max_in", _lib.IO_SCALAR_IN, loop)) if isinstance(max_in, str) else Scalar.const(max_in)
    p.add_op(_lib.OP_HISTOGRAM_STATS, src=0, ip=(1, 0), sp=(mi,))
    for k, name in enumerate(("mode", "max", "fwhm")):
        p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io(name, _lib.IO_SCALAR_OUT, loop), ip=(k,))
    return p


# ------------------------------------------------------------------------------------------------------------------------------------
# the fragment of the reference's SiPM recipes that the two processors serve
# ------------------------------------------------------------------------------------------------------------------------------------
_M = "dspeed.processors"


def sipm_fragment(source="waveform", lists=20):
    """avg_current -> histogram -> histogram_stats -> get_multi_local_extrema with 3*fwhm, in the module strings of the reference's SiPM recipes"""
    return {
        "curr": {"function": "avg_current", "module": f"{_M}.moving_windows", "args": [source, 5, f"curr(len({source})-5)"], "unit": "ADC"},
        "hist_weights , hist_borders": {"function": "histogram", "module": f"{_M}.histogram", "args": ["curr", "hist_weights(100)", "hist_borders(101)"],
                                        "unit": ["none", "ADC"]},
        "fwhm, idx_out_c, max_out": {"function": "histogram_stats", "module": f"{_M}.histogram",
                                     "args": ["hist_weights", "hist_borders", "idx_out_c", "max_out", "fwhm", "np.nan"], "unit": ["ADC", "non", "ADC"]},
        "vt_max_candidate_out, vt_min_out, n_max_out, n_min_out": {
            "function": "get_multi_local_extrema", "module": f"{_M}.get_multi_local_extrema",
            "args": ["curr", 5, 0.1, 1, "3*fwhm", 0, f"vt_max_candidate_out({lists}, vector_len=n_max_out)", f"vt_min_out({lists}, vector_len=n_min_out)",
                     "n_max_out", "n_min_out"], "unit": ["ns", "ns", "none", "none"]}}


def sipm_rows(n_rows=24, n=1000, seed=0x51B):
    """uint16 rows: a baseline with noise and a few sharp pulses of different heights, so that 3 * fwhm of the current's histogram passes some
    maxima and stops others"""
    rng = np.random.default_rng(seed)
    w = 2000 + np.rint(4 * rng.standard_normal((n_rows, n)))
    for r in range(n_rows):
        for _ in range(int(rng.integers(0, 6))):
            at, height = int(rng.integers(20, n - 60)), float(rng.choice([15, 40, 120, 400]))
            w[r, at:] += np.rint(height * np.exp(-np.arange(n - at) / 30.0))
    return w.astype(np.uint16)
