"""Cases of get_multi_local_extrema (dsp_extrema.hip): the rows and parameters tools/gen_golden_extrema.py feeds to the reference's body
(tests/golden/get_multi_local_extrema.npz holds them with what the body returned), what test_extrema_cases_cpu.py asks of them, and a NumPy
model of the kernel's formulation -- groups of 64 N samples, N per lane, a prefix inside the lane and one across the lanes -- that the same
test holds against the fixtures before anything runs on a GPU.  Nothing here needs a GPU or the reference.  Every row comes from a seed."""
import numpy as np

BOOK = "get_multi_local_extrema"
KERNEL = "get_multi_local_extrema"
#: samples per lane the kernels are built with: 1 (unaligned rows), 2 (float64), 4 (float32, int32, uint32), 8 (int16, uint16)
LANE_SAMPLES = (1, 2, 4, 8)
UNION_MAX = 64  # search_direction 3: the longest list the kernel takes (DSP_EXTREMA_UNION_MAX)
LENGTHS = (3, 63, 64, 65, 130, 255, 256, 257, 511, 513, 8192)  # (130: no multiple of 4)


# ------------------------------------------------------------------------------------------------------------------------------------
# rows, in sweep order
# ------------------------------------------------------------------------------------------------------------------------------------
def zigzag(n, events):
    """A row (in sweep order) on which a delta of 5 tags exactly the extremes e at the trigger samples t of ``events`` = [(e, t), ...],
    maxima and minima in turn, prev t < e < t: 10 at a maximum, 8 until its trigger, 0 on it; -10 / -8 / 0 for a minimum; +-2 in between."""
    w = np.zeros(n, dtype=np.float32)
    at, sign = 0, 1.0
    for e, t in events:
        assert at <= e < t < n, (events, n)
        w[at:e] = 2 * sign
        w[e] = 10 * sign
        w[e + 1:t] = 8 * sign
        w[t] = 0
        at, sign = t + 1, -sign
    w[at:] = 2 * sign
    return w


def spread_events(n, count, first=1):
    """``count`` events spread evenly over a row of n samples"""
    step = max(2, (n - first) // max(count, 1))
    return [(first + k * step, first + k * step + max(1, step // 2)) for k in range(count) if first + k * step + max(1, step // 2) < n]


def _rows_for(n, rng):
    """[(name, row in sweep order, a_delta_max, a_delta_min, a_abs_max, a_abs_min)]"""
    inf = np.inf
    rows = []
    if n >= 8:
        ev = spread_events(n, min(24, n // 4))
        rows.append(("zigzag", zigzag(n, ev), 5, 5, -inf, inf))
        # the same row with thresholds that let the maxima pass (10 > 9) and no minimum (-10 < -11 is false) ...
        rows.append(("zigzag_abs_min", zigzag(n, ev), 5, 5, 9, -11))
        # ... and with one that stops the machine at its first maximum
        rows.append(("zigzag_abs_max", zigzag(n, ev), 5, 5, 10, inf))
        # several transitions within one group of 64, the rest of the row quiet
        rows.append(("burst", zigzag(n, [(1, 2), (3, 4), (5, 6), (7, 8)][: max(1, (n - 1) // 2)]), 5, 5, -inf, inf))
        # a tied maximum: two samples of 10, the first in sweep order is the one tagged
        w = zigzag(n, ev[:2] if len(ev) >= 2 else ev)
        e, t = ev[0]
        if t - e >= 2:
            w[t - 1] = 10
        rows.append(("tie", w, 5, 5, -inf, inf))
        # a transition on the last sample: the last, partial group
        rows.append(("last_sample", zigzag(n, [(n // 3, n - 1)]), 5, 5, -inf, inf))
        # infinite samples: the maximum +inf, the minimum -inf
        w = zigzag(n, ev[:4])
        w[ev[0][0]] = inf
        if len(ev) > 1:
            w[ev[1][0]] = -inf
        rows.append(("inf", w, 5, 5, -inf, inf))
    if n >= 513:  # triggers at sweep positions 63 / 0 modulo 64, 255 / 0 modulo 256, 511 / 0 modulo 512; extremes groups ahead of their triggers
        rows.append(("edges_a", zigzag(n, [(100, 127), (150, 192), (300, 511)]), 5, 5, -inf, inf))
        rows.append(("edges_b", zigzag(n, [(10, 63), (70, 128), (200, 256), (300, 512)]), 5, 5, -inf, inf))
    elif n >= 257:
        rows.append(("edges_a", zigzag(n, [(10, 63), (70, 128), (200, 255)]), 5, 5, -inf, inf))
        rows.append(("edges_b", zigzag(n, [(20, 127), (130, 192), (200, 256)][: 3 if n > 256 else 2]), 5, 5, -inf, inf))
    elif n >= 65:
        rows.append(("edges_a", zigzag(n, [(10, 63)]), 5, 5, -inf, inf))
        rows.append(("edges_b", zigzag(n, [(10, 64)]), 5, 5, -inf, inf))
    # nothing to find: a constant row, a rising one
    rows.append(("constant", np.full(n, 3, dtype=np.float32), 1, 1, -inf, inf))
    rows.append(("rising", np.arange(n, dtype=np.float32), 1, 1, -inf, inf))
    # noise, integer-valued noise with ties, a random walk of integer steps, a rounded sine
    rows.append(("noise", rng.standard_normal(n).astype(np.float32), 0.5, 0.7, -0.2, 0.3))
    rows.append(("noise_delta0", rng.standard_normal(n).astype(np.float32), 0, 0, -inf, inf))
    rows.append(("ties", rng.integers(-3, 4, n).astype(np.float32), 2, 1, -inf, inf))
    rows.append(("ties_delta0", rng.integers(-2, 3, n).astype(np.float32), 0, 0, -inf, inf))
    rows.append(("walk", np.cumsum(rng.integers(-2, 3, n)).astype(np.float32), 3, 2, -inf, inf))
    rows.append(("sine", np.rint(20 * np.sin(np.arange(n) * (2 * np.pi / 37.0)) + rng.integers(-1, 2, n)).astype(np.float32), 6, 6, 5, -5))
    # the NaN rule: a NaN in the first and in the last sample, a NaN delta
    for name, where in (("nan_first", 0), ("nan_last", n - 1)):
        w = rng.integers(-3, 4, n).astype(np.float32)
        w[where] = np.nan
        rows.append((name, w, 1, 1, -inf, inf))
    rows.append(("nan_delta_max", rng.integers(-3, 4, n).astype(np.float32), np.nan, 1, -inf, inf))
    rows.append(("nan_delta_min", rng.integers(-3, 4, n).astype(np.float32), 1, np.nan, -inf, inf))
    rows.append(("nan_abs", rng.integers(-3, 4, n).astype(np.float32), 1, 1, np.nan, np.nan))
    return rows


def _ms(n):
    return sorted({m for m in (1, 2, 5, 20, n - 1) if m < n})


class Group:
    """rows of one length that go through one launch: ``w`` (R, n) in the rows' own type, the four parameter columns in the loop's type, the
    rows' names, and the (search_direction, m) pairs the reference ran"""

    def __init__(self, name, tag, w, par, names, combos, extra=None):
        self.name, self.tag, self.w, self.par, self.names, self.combos = name, tag, w, par, names, combos
        self.loop = np.float32 if tag == "f32" else np.float64
        self.extra = dict(extra or {})  # further arrays of the case (what a recipe computes the rows and parameters from)


RECIPE_N, RECIPE_ROWS, RECIPE_TAU, RECIPE_FIT = 512, 18, 400.0, 100


def recipe_groups():
    """The rows of the recipe tests (test_gpu_extrema.py).  ``rcp``: oscillating float32 rows with the constants of the reference's own test
    recipe (tests/test_processing_chain.py:263-286: deltas 5, a_abs_max 10, a_abs_min 0).  ``rcppz``: int16 pile-up pulses that a recipe
    baseline-subtracts and pole-zero corrects first; the case's rows are the ORACLE's pole_zero output and its parameters what the recipe
    forms from the oracle's linear_slope_fit of the baseline (5 * bl_std, bl_std, bl_mean + 3 * bl_std, 0), in float32 as the device does."""
    import oracle

    rng = np.random.default_rng(4242)
    i = np.arange(RECIPE_N, dtype=np.float64)
    names = [f"row{k}" for k in range(RECIPE_ROWS)]
    wave = np.rint(25 * np.sin(i[None, :] * (2 * np.pi / 97.0) + rng.uniform(0, 6.28, (RECIPE_ROWS, 1))) + 3 * rng.standard_normal((RECIPE_ROWS, RECIPE_N)))
    par = np.tile(np.array([[5.0], [5.0], [10.0], [0.0]], dtype=np.float32), (1, RECIPE_ROWS))
    out = [Group(f"rcp_n{RECIPE_N}", "f32", wave.astype(np.float32), par, names, [(0, 10), (0, 20), (1, 10), (1, 20)])]
    raw = rng.uniform(900, 1100, (RECIPE_ROWS, 1)) + 4 * rng.standard_normal((RECIPE_ROWS, RECIPE_N))
    for _ in range(3):  # three pulses a row, behind the baseline window
        t0 = rng.integers(160, 440, (RECIPE_ROWS, 1))
        raw += rng.uniform(100, 1500, (RECIPE_ROWS, 1)) * np.exp(-(i[None, :] - t0) / RECIPE_TAU) * (i[None, :] >= t0)
    raw = np.rint(raw).astype(np.int16)
    baseline = np.rint(raw[:, :50].mean(axis=1)).astype(np.float32)
    blsub, rc = oracle.bl_subtract(raw.astype(np.float32), baseline)
    assert rc == 0
    pz, rc = oracle.pole_zero(blsub, RECIPE_TAU)
    assert rc == 0
    mean, std, _slope, _intercept, rc = oracle.linear_slope_fit(np.ascontiguousarray(blsub[:, :RECIPE_FIT]))
    assert rc == 0
    f = np.float32
    par = np.stack([f(5) * std, std, f(3) * std + mean, np.zeros_like(std)]).astype(np.float32)
    out.append(Group(f"rcppz_n{RECIPE_N}", "f32", pz, par, names, [(0, 20), (1, 20)], extra={"raw": raw, "baseline": baseline}))
    return out


def groups():
    out = []
    for n in LENGTHS:
        rng = np.random.default_rng(7000 + n)
        rows = _rows_for(n, rng)
        if n == 8192:  # (the book's size: the crafted rows and two of the others)
            rows = [r for r in rows if r[0] in ("zigzag", "burst", "tie", "edges_a", "edges_b", "last_sample", "inf", "noise", "walk", "nan_last")]
        # every row as it stands (forward sweeps find what it was built for) and reversed (backward sweeps do)
        w = np.stack([r[1] for r in rows] + [r[1][::-1] for r in rows])
        par = np.array([r[2:] for r in rows] * 2, dtype=np.float32).T.copy()
        names = [r[0] for r in rows] + [r[0] + "_rev" for r in rows]
        ms = _ms(n) if n != 8192 else [5, 20, 8191]
        combos = [(d, m) for d in (0, 1, 3) for m in ms if d != 3 or m <= UNION_MAX]
        out.append(Group(f"f32_n{n}", "f32", w, par, names, combos))
    # integer rows: the int16 / uint16 copies of integer-valued rows (the float32 loop), int32 / uint32 and float64 (the float64 loop)
    for n in (65, 513):
        rng = np.random.default_rng(9000 + n)
        rows = [r for r in _rows_for(n, rng) if r[0] in ("zigzag", "burst", "tie", "edges_a", "edges_b", "last_sample", "ties", "ties_delta0", "walk", "sine")]
        w = np.stack([r[1] for r in rows] + [r[1][::-1] for r in rows])
        par = np.array([r[2:] for r in rows] * 2, dtype=np.float64).T.copy()
        names = [r[0] for r in rows] + [r[0] + "_rev" for r in rows]
        combos = [(d, m) for d in (0, 1, 3) for m in (2, 20)]
        out.append(Group(f"i16_n{n}", "f32", w.astype(np.int16), par.astype(np.float32), names, combos))
        out.append(Group(f"u16_n{n}", "f32", (w + 1000).astype(np.uint16), (par + np.array([[0], [0], [1000], [1000]])).astype(np.float32), names, combos))
        out.append(Group(f"i32_n{n}", "f64", (w * 100000).astype(np.int32), par * 100000, names, combos))
        out.append(Group(f"u32_n{n}", "f64", ((w + 1000) * 100000).astype(np.uint32), (par + np.array([[0], [0], [1000], [1000]])) * 100000, names, combos))
        noise = np.random.default_rng(9500 + n).standard_normal((4, n))
        npar = np.array([[0.5, 0.7, -0.2, 0.3], [0, 0, -np.inf, np.inf], [1e-9, 1e-9, -np.inf, np.inf], [2.0, 0.1, 0.5, 0.0]]).T.copy()
        out.append(Group(f"f64_n{n}", "f64", np.concatenate([noise, w.astype(np.float64) / 3]), np.concatenate([npar, par / 3], axis=1),
                         ["noise%d" % k for k in range(4)] + names, combos))
    return out + recipe_groups()


def key(direction, m, what):
    return f"d{direction}_m{m}_{what}"


# ------------------------------------------------------------------------------------------------------------------------------------
# what the reference's outputs say about a row
# ------------------------------------------------------------------------------------------------------------------------------------
def sweep_events(w, direction, d_max, d_min, vt_max, vt_min):
    """[(is_max, position of the tagged extreme, position of the sample that triggered it)] in sweep order, from the lists the reference
    returned for one row and one sweep (direction 0 or 1): maxima and minima alternate, a maximum first; the trigger of an extreme at
    position e is the first sample behind e that lies more than delta beyond it (the comparison of reference lines 147 / 159, in the
    loop's type)."""
    n = len(w)
    x = w if direction == 0 else w[::-1]
    tags = [[int(v) for v in vt[~np.isnan(vt)]] for vt in (vt_max, vt_min)]
    events, k, is_max = [], [0, 0], True
    while k[0 if is_max else 1] < len(tags[0 if is_max else 1]):
        index = tags[0 if is_max else 1][k[0 if is_max else 1]]
        e = index if direction == 0 else n - 1 - index
        with np.errstate(invalid="ignore"):
            beyond = (x[e + 1:] < x[e] - d_max) if is_max else (x[e + 1:] > x[e] + d_min)
        assert beyond.any(), "a tagged extreme without a trigger behind it"
        events.append((is_max, e, e + 1 + int(np.argmax(beyond))))
        k[0 if is_max else 1] += 1
        is_max = not is_max
    return events


# ------------------------------------------------------------------------------------------------------------------------------------
# the kernel's formulation in NumPy
# ------------------------------------------------------------------------------------------------------------------------------------
def model_sweep(x, m, d_max, d_min, a_max, a_min, lane_samples):
    """one sweep over ``x`` (already in sweep order, in the loop's type): the positions tagged as maxima and as minima"""
    T = x.dtype.type
    n, N = len(x), lane_samples
    G = 64 * N
    mx, rv, rp = True, x[0], 0
    tags = ([], [])
    for base in range(0, n, G):
        pos = base + np.arange(G)
        xs = np.zeros(G, dtype=x.dtype)
        xs[: min(G, n - base)] = x[base:base + G]
        q = -1
        while True:
            with np.errstate(invalid="ignore"):
                y = xs if mx else -xs
                alive = (pos > q) & (pos < n)
                # the lane's own prefix: strict comparisons, the first occurrence stays
                lv = np.empty((64, N), dtype=x.dtype)
                lp = np.zeros((64, N), dtype=np.int64)
                cv = np.full(64, -np.inf, dtype=x.dtype)
                cp = np.zeros(64, dtype=np.int64)
                ya, al, po = y.reshape(64, N), alive.reshape(64, N), pos.reshape(64, N)
                for j in range(N):
                    t = al[:, j] & (ya[:, j] > cv)
                    cv = np.where(t, ya[:, j], cv)
                    cp = np.where(t, po[:, j], cp)
                    lv[:, j], lp[:, j] = cv, cp
                # the lanes' totals across the wavefront, the running extreme carried in at lane 0; ev / ep: what the lane below holds
                tv, tp = cv.copy(), cp.copy()
                if not tv[0] > rv:
                    tv[0], tp[0] = rv, rp
                run = np.maximum.accumulate(tv)  # (lane l keeps its own total only where it lies above everything below it)
                own = np.ones(64, dtype=bool)
                own[1:] = tv[1:] > run[:-1]
                tv, tp = run, tp[np.maximum.accumulate(np.where(own, np.arange(64), 0))]
                ev = np.concatenate([[rv], tv[:-1]]).astype(x.dtype)
                ep = np.concatenate([[rp], tp[:-1]])
                later = lv > ev[:, None]
                pv = np.where(later, lv, ev[:, None])
                pp = np.where(later, lp, ep[:, None])
                d, a = (T(d_max), T(a_max)) if mx else (T(d_min), -T(a_min))
                room = len(tags[0 if mx else 1]) < m
                trig = al & room & (ya < pv - d) & (pv > a)
            if not trig.any():
                rv, rp = tv[63], tp[63]
                break
            first = int(np.argmax(trig.reshape(-1)))
            tags[0 if mx else 1].append(int(pp.reshape(-1)[first]))
            q = int(pos[first])
            rv, rp = -y[first], q
            mx = not mx
    return tags


def model(w, d_max, d_min, direction, a_max, a_min, m, loop, lane_samples):
    """(vt_max, vt_min, n_max, n_min) of one row as the kernel forms them"""
    x = np.asarray(w).astype(loop)
    d_max, d_min, a_max, a_min = (loop(v) for v in (d_max, d_min, a_max, a_min))
    out = [np.full(m, np.nan, dtype=loop), np.full(m, np.nan, dtype=loop)]
    counts = [0, 0]
    if not (np.isnan(x).any() or np.isnan(d_max) or np.isnan(d_min)):
        n = len(x)
        fwd = model_sweep(x, m, d_max, d_min, a_max, a_min, lane_samples) if direction in (0, 3) else ([], [])
        bwd = model_sweep(x[::-1].copy(), m, d_max, d_min, a_max, a_min, lane_samples) if direction in (1, 3) else ([], [])
        bwd = tuple([n - 1 - p for p in tags] for tags in bwd)
        for k in range(2):
            if direction == 3:
                found = sorted(set(fwd[k]) | set(bwd[k]))[:m]
            else:
                found = fwd[k] if direction == 0 else bwd[k]
            out[k][: len(found)] = found
            counts[k] = len(found)
    return out[0], out[1], np.uint32(counts[0]), np.uint32(counts[1])
