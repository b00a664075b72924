"""The run-length FIR (dsp_fir_runs.hip) at every step, window and group edge: the kernel's geometry restated as small pure functions, the
cases made from them by rule, and two families of rows and taps for every case -- for tests/test_gpu_fir_runs_cases.py (the device) and
tests/test_fir_runs_cases_cpu.py (is the list what it claims? -- the planner, the oracle and NumPy alone).  Nothing here needs a GPU; every
row and tap comes from a seed.

A kernel is written as its runs, ``(kind, length)`` with kind 'v' (a value of its own), '0' (zeros) or '=' (the value of the run before:
two neighbouring runs without a breakpoint between them); ``breakpoints`` then finds what the prep kernel finds in the taps themselves.

The exact family makes an off-by-one anywhere an inequality of integers: run values are distinct integers of alternating sign with the
largest at both ends, rows are small integers, every prefix sum, weight and product is an integer and every output lies below 2^24 -- the
expectation is the int64 convolution, compared with ``np.array_equal``, and the per-event values are the oracle's on that expectation.
The pedestal family catches what integers cannot, a prefix sum, weight or carry held in float32: rows 1000 + uniform(-1, 1) with full
significands under run values in +-[0.5, 1], against the float64 convolution at 1e-6 of the row's filtered peak."""
import functools

import numpy as np

import oracle

M = "dspeed.processors"
TOL = 1e-6  # of the row's filtered peak (test_gpu_fir_runs.py)
TAPS_FILE = "mem:fir_runs_taps"  # (a recipe reads its taps with loadlh5(TAPS_FILE, '<family>/<case id>'))
MODES = {"v": "valid", "s": "same", "f": "full"}
PEDESTAL = 1000.0
SENTINEL = np.float32(-7777.25)  # what a kept output's buffer holds before the launch

# ------------------------------------------------------------------------------------------------------------------------------------
# geometry (dsp_fir_runs.hip, dsp_plan.cpp, dsp_kernels.h, dsp_program.h)
# ------------------------------------------------------------------------------------------------------------------------------------
STEP = 512                 # dsp_kernels.h:71
PSTEP = STEP + STEP // 8   # dsp_fir_runs.hip:111
RUNS_MAX, MAX_TAPS, GROUP = 24, 512, 8  # dsp_program.h:370-372


def out_len(mode, m, n):
    """dsp_plan.cpp:824"""
    return {"v": n - m + 1, "s": n, "f": n + m - 1}[mode]


def start(mode, m):
    """dsp_plan.cpp:857: output c of the kernel is np.convolve(x, k, 'full')[c + start]"""
    return {"v": m - 1, "s": (m - 1) // 2, "f": 0}[mode]


def mp(m):
    """dsp_fir_runs.hip:110"""
    return (m + 63) & ~63


def pmp(m):
    """dsp_fir_runs.hip:112"""
    return mp(m) + mp(m) // 8


def n_steps(mode, m, n):
    """dsp_fir_runs.hip:132"""
    return (out_len(mode, m, n) + start(mode, m) + STEP - 1) // STEP


def input_step_full(g, n):
    """dsp_fir_runs.hip:158"""
    return g * STEP + STEP <= n


def output_step_vector(g, st, p, lo=0, hi=0):
    """dsp_fir_runs.hip:202 (``lo`` / ``hi``: the predicate off by that much at either end, for the CPU test's mutations)"""
    return g * STEP - st >= -lo and g * STEP - st + STEP <= p + hi


def window_index(i):
    """dsp_fir_runs.hip:92, 175: sum i lives at element i + i / 8"""
    return i + i // 8


def lds_bytes(m):
    """dsp_kernels.h:72-75"""
    return (4 * (pmp(m) + PSTEP) + 64) * 8


def scratch_pitch(p):
    """dsp_plan.cpp:858"""
    return (p + 63) & ~63


def breakpoints(taps):
    """the prep kernel, dsp_fir_runs.hip:49-69 -> (t, weight, raw count, finite): every tap index in [0, m] where the kernel differs from
    the tap before (zeros in front and behind), compared in float32 as the device does (-0.0 equals 0.0, a NaN differs from everything)"""
    k = np.asarray(taps, dtype=np.float32)
    m = len(k)
    cur, prev = np.concatenate([k, [np.float32(0)]]), np.concatenate([[np.float32(0)], k])
    with np.errstate(invalid="ignore"):
        brk = cur != prev
        finite = bool((k - k == 0).all())
    t = np.flatnonzero(brk)
    assert t.size == 0 or t[-1] <= m
    return t, cur[t].astype(np.float64) - prev[t].astype(np.float64), int(t.size), finite


def table(taps):
    """what the kernel reads (dsp_fir_runs.hip:66-69): (t, weight) of the sum path, or None where every row is done tap by tap -- taps that
    are not finite, more than RUNS_MAX + 1 breakpoints, or none at all"""
    t, w, raw, finite = breakpoints(taps)
    if not finite or raw > RUNS_MAX + 1 or raw == 0:
        return None
    return t, w


def groups(t):
    """dsp_fir_runs.hip:71-78: breakpoints at consecutive taps go together, GROUP at the most -> [(first entry, count)]"""
    out, b = [], 0
    while b < len(t):
        cnt = 1
        while b + cnt < len(t) and cnt < GROUP and t[b + cnt] == t[b] + cnt:
            cnt += 1
        out.append((b, cnt))
        b += cnt
    return out


def ramps(t):
    """lengths of the maximal runs of consecutive breakpoints"""
    out, b = [], 0
    while b < len(t):
        cnt = 1
        while b + cnt < len(t) and t[b + cnt] == t[b] + cnt:
            cnt += 1
        out.append(cnt)
        b += cnt
    return out


def admitted(n, m, mode, dtype=np.float32, offset=0, stride=None):
    """the planner's admission, dsp_plan.cpp:812-825 (the hint set, float32 compute)"""
    stride = n + offset if stride is None else stride
    if np.dtype(dtype) != np.float32 or n % 8 or n < 8 or stride % 4 or offset % 4:
        return False
    return 1 <= m <= min(n, MAX_TAPS) and out_len(mode, m, n) >= 1


def steps_of(mode, m, n):
    """per step g: (first output, 'vector' | 'start' | 'p' | 'both' | 'none')"""
    st, p = start(mode, m), out_len(mode, m, n)
    out = []
    for g in range(n_steps(mode, m, n)):
        c0 = g * STEP - st
        if output_step_vector(g, st, p):
            kind = "vector"
        else:
            kind = {(True, True): "both", (True, False): "start", (False, True): "p", (False, False): "none"}[(c0 < 0, c0 + STEP > p)]
        out.append((c0, kind))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------
def V(*lens):
    return tuple(("v", int(l)) for l in lens)


def group_runs(G, pos, m):
    """G consecutive breakpoints starting at tap 0 ('front'), ending at tap m ('end') or away from both ('middle')"""
    if pos == "front":
        return V(*([1] * (G - 1) + [m - (G - 1)]))
    if pos == "end":
        return V(*([m - (G - 1)] + [1] * (G - 1)))
    a = 11
    return V(*([a] + [1] * (G - 1) + [m - a - (G - 1)]))


class Case:
    """``why``: the class the case is in the list for (it is in ``classes(case)``); ``runs``: the kernel; ``n``: samples a row; ``pattern``:
    what the rows are ('std', 'extremes', 'nonfinite', 'rounds'); ``tap_nan``: a NaN put into the taps; ``off`` / ``stride``: where the kept
    output lies in its buffer (elements)"""

    def __init__(self, why, mode, runs, n, rows=5, off=0, pattern="std", tap_nan=False, recipe=False):
        self.why, self.mode, self.runs, self.n, self.rows, self.off, self.pattern, self.tap_nan, self.recipe = why, mode, tuple(runs), n, rows, off, pattern, tap_nan, recipe
        self.m = sum(l for _, l in self.runs)
        self.P = out_len(mode, self.m, n)
        self.start = start(mode, self.m)
        self.stride = self.P + 8 if off == 0 else (self.P + off + 8) | 1  # (an odd stride under the offsets 1, 2, 3)
        self.id = None
        assert admitted(n, self.m, mode), (why, mode, self.m, n)

    @property
    def layout(self):
        """the breakpoints of the layout (every 'v' run differs from its neighbours, in both families)"""
        return breakpoints(taps_of(self.runs, "exact"))

    @property
    def sum_path(self):
        return not self.tap_nan and table(taps_of(self.runs, "exact")) is not None

    @property
    def families(self):
        return ("exact", "pedestal") if self.sum_path and self.pattern in ("std", "rounds") else ("exact",)


def kernel_shape(c):
    t, _, raw, _ = c.layout
    if raw == 2 and t[0] == 0 and t[1] == c.m:
        return "boxcar"
    if raw == 3 and t[0] == 0 and t[2] == c.m:
        return "two runs"
    return None


def classes(c):
    """the names of the classes the case belongs to, from its geometry"""
    m, n, mode, P, st = c.m, c.n, c.mode, c.P, c.start
    t, _, raw, _ = c.layout
    out = [f"rows {c.rows}" if c.pattern != "rounds" else "many rounds", f"m={m}", f"n={n}", f"n_steps={n_steps(mode, m, n)}", f"P%64={P % 64}",
           f"start%8={st % 8}", f"kept offset {c.off}", f"breakpoints {raw}", f"pattern {c.pattern}"]
    if c.tap_nan:
        return tuple(out + ["a NaN tap"])
    if not any(k == "v" for k, _ in c.runs):
        out.append("all-zero kernel: tap by tap")
    elif raw > RUNS_MAX + 1:
        out.append(f"{raw} breakpoints: tap by tap")
    else:
        for b, G in groups(t):
            s = mp(m) - t[b] - (G - 1)
            pos = [w for w, hit in (("front", t[b] == 0), ("end", t[b + G - 1] == m)) if hit] or ["middle"]
            out += [f"G={G} {w}" for w in pos]
            if s == 0:
                out.append(f"s=0 G={'1' if G == 1 else '>1'}")
        out += [f"ramp {L}" for L in ramps(t) if L > GROUP]
        if m == mp(m) and t[-1] == m:
            out.append("m == mp: the last breakpoint reads window element 0")
    kinds = [k for k, _ in c.runs]
    out += ["leading zero taps"] if kinds[0] == "0" and "v" in kinds else []
    out += ["trailing zero taps"] if kinds[-1] == "0" and "v" in kinds else []
    out += ["zero run in the middle"] if "0" in kinds[1:-1] else []
    out += ["equal neighbouring runs"] if "=" in kinds else []
    shape = kernel_shape(c)
    out += [f"m={m} {shape}"] if shape else []
    # input steps
    last = (n - 1) // STEP
    out.append(f"last input step {(n - last * STEP) // 8} live lanes")
    if n_steps(mode, m, n) * STEP - STEP >= n:
        out.append("a step wholly behind the row's end")
    # output steps
    for g, (c0, kind) in enumerate(steps_of(mode, m, n)):
        out.append({"vector": f"{mode} step on the vector-store path", "start": f"{mode} first step cut by start", "p": f"{mode} last step cut by p",
                    "both": f"{mode} step cut at both ends", "none": f"{mode} step without an output"}[kind])
        if output_step_vector(g, st, P, lo=1) and not output_step_vector(g, st, P):
            out.append("vector predicate: one output short at the start")
        if output_step_vector(g, st, P, hi=1) and not output_step_vector(g, st, P):
            out.append("vector predicate: one output short at the end")
    if mode == "s":
        out.append("s odd m" if m & 1 else "s even m")
    if P == 1:
        out.append("p=1")
    return tuple(dict.fromkeys(out))


NS = (8, 16, 504, 512, 520, 1024, 1032, 1536, 1544, 3072, 3080)
WINDOW_MS = (1, 8, 63, 64, 65, 127, 128, 129, 448, 449, 511, 512)


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(why, mode, runs, n, **kw):
        out.append(Case(why, mode, runs, n, **kw))

    # ---- group size: G = 1 .. 8 at the front, at the end and in the middle of a 40-tap kernel (mp = 64); modes and lengths in turn
    turn = (("s", 520), ("v", 1032), ("f", 512))
    for i, (G, pos) in enumerate((G, pos) for G in range(1, 9) for pos in ("front", "end", "middle")):
        mode, n = turn[(i + i // 3) % 3]
        add(f"G={G} {pos}", mode, group_runs(G, pos, 40), n, recipe=(G, pos) in ((3, "front"), (5, "middle"), (7, "end")))
    # ramps longer than a group: 8 + 1, 8 + 8, 8 + 8 + 1
    for i, L in enumerate((9, 16, 17)):
        add(f"ramp {L}", "svf"[i], V(*([10] + [1] * (L - 1) + [48 - 10 - (L - 1)])), (1032, 520, 520)[i], recipe=L in (9, 17))
    # a ramp that ends at m, m a multiple of 64: the group's first window element is element 0
    add("s=0 G=>1", "s", V(*([57] + [1] * 7)), 1032, recipe=True)
    add("s=0 G=1", "f", V(*([120] + [1] * 8)), 520)
    # ---- the table
    add("breakpoints 2", "s", V(24), 520, recipe=True)
    add("breakpoints 3", "v", V(9, 15), 520)
    add("breakpoints 24", "s", V(*[2 + i % 3 for i in range(23)]), 1032)
    add("breakpoints 25", "f", V(*[2 + i % 3 for i in range(24)]), 520, recipe=True)
    add("breakpoints 25", "v", V(*([3] * 8 + [1] * 8 + [4] * 8)), 1032)  # (with a group of 8 and one of 1 in it)
    add("26 breakpoints: tap by tap", "s", V(*[2 + i % 3 for i in range(25)]), 520, recipe=True)
    add("leading zero taps", "s", (("0", 5), ("v", 10), ("v", 12)), 520, recipe=True)
    add("trailing zero taps", "f", (("v", 10), ("v", 12), ("0", 5)), 520, recipe=True)
    add("zero run in the middle", "v", (("v", 10), ("0", 6), ("v", 12)), 520)
    add("equal neighbouring runs", "s", (("v", 10), ("=", 7), ("v", 9)), 520)
    add("m=1", "s", V(1), 520, recipe=True)
    add("all-zero kernel: tap by tap", "s", (("0", 16),), 520)
    # ---- the window: boxcars and two runs, so that the last breakpoint sits at m
    for i, m in enumerate(WINDOW_MS):
        mode = "fsv"[i % 3]
        n = 512 if m == 512 else 520  # ('f' with n = m = 512: the second step lies wholly behind the row's end)
        add(f"m={m} boxcar", mode, V(m), n)
        if m > 1:
            add(f"m={m} two runs", "svf"[i % 3], V(m // 3 + 1, m - m // 3 - 1), n if m < 512 else 1032)
    # ---- input steps: every length in every mode (n_steps 1 .. 7 with them), a 12-tap kernel with a group of 2 in the middle
    for n in NS:
        for mode in "svf":
            if admitted(n, 12, mode):
                add(f"n={n}", mode, V(4, 1, 7), n)
    add("n=8", "f", V(3, 1, 4), 8)
    add("n_steps=5", "f", V(200, 312), 1544)
    # ---- output steps
    for m in range(1, 9):  # start % 8 = 0 .. 7 under 'v'; m = 2: the first step is one output short of the vector path
        add(f"start%8={(m - 1) % 8}", "v", V(m) if m < 3 else V(1, m - 1), 1032)
    add("vector predicate: one output short at the end", "f", V(3, 5), 504)
    add("p=1", "v", V(3, 5), 8)
    add("p=1", "v", V(100, 412), 512)
    for mode in "vs":
        add(f"{mode} step cut at both ends", mode, V(4, 1, 7), 504)
    for off in (1, 2, 3):
        add(f"kept offset {off}", "s", V(4, 1, 7), 1032, off=off)
    add("kept offset 1", "v", V(2), 1032, off=1)  # (what the start-short vector predicate would write lies in front of the row)
    # ---- P % 64 (the pitch of the scratch rows)
    add("P%64=1", "f", V(2), 512)
    add("P%64=63", "v", V(2), 512)
    # ---- rows a launch
    for rows in (1, 3, 4):
        add(f"rows {rows}", "s", V(4, 1, 7), 520, rows=rows)
    add("many rounds", "s", V(9, 1, 1, 21), 64, rows=0, pattern="rounds")
    # ---- extremes in flight
    add("pattern extremes", "s", V(8), 1544, rows=6, pattern="extremes")
    add("pattern extremes", "v", V(8), 1544, rows=6, pattern="extremes")
    # ---- NaN and infinities among the samples, a NaN among the taps
    add("pattern nonfinite", "s", V(4, 1, 7), 520, rows=6, pattern="nonfinite")
    add("pattern nonfinite", "f", (("v", 10), ("0", 6), ("v", 12)), 1032, rows=6, pattern="nonfinite")
    add("a NaN tap", "s", V(4, 1, 7), 520, tap_nan=True)
    for i, c in enumerate(out):
        c.id = f"{i:03d}-{c.mode}-{c.m}taps-{c.layout[2]}bp-{c.n}x{c.rows}" + (f"-at{c.off}" if c.off else "") + ("" if c.pattern == "std" else f"-{c.pattern}") + ("-nantap" if c.tap_nan else "")
    return tuple(out)


@functools.lru_cache(maxsize=None)
def by_id(case_id):
    return next(c for c in cases() if c.id == case_id)


#: every class the list must hit (test_fir_runs_cases_cpu.py holds the list against it)
CLASSES = tuple(
    [f"G={G} {pos}" for G in range(1, 9) for pos in ("front", "end", "middle")] + ["ramp 9", "ramp 16", "ramp 17", "s=0 G=>1", "s=0 G=1"] +
    [f"breakpoints {b}" for b in (0, 2, 3, 24, 25, 26)] + ["26 breakpoints: tap by tap", "all-zero kernel: tap by tap", "leading zero taps", "trailing zero taps",
     "zero run in the middle", "equal neighbouring runs", "m=1", "m == mp: the last breakpoint reads window element 0"] +
    [f"m={m} boxcar" for m in WINDOW_MS] + [f"m={m} two runs" for m in WINDOW_MS if m > 1] + [f"n={n}" for n in NS] + [f"n_steps={k}" for k in range(1, 8)] +
    [f"last input step {k} live lanes" for k in (1, 63, 64)] + ["a step wholly behind the row's end"] +
    [f"{mode} step on the vector-store path" for mode in "svf"] + ["s first step cut by start", "v first step cut by start"] +
    [f"{mode} last step cut by p" for mode in "svf"] + [f"{mode} step cut at both ends" for mode in "sv"] + [f"start%8={k}" for k in range(8)] +
    ["vector predicate: one output short at the start", "vector predicate: one output short at the end", "s odd m", "s even m", "p=1"] +
    [f"kept offset {k}" for k in range(4)] + [f"P%64={k}" for k in (0, 1, 63)] + [f"rows {k}" for k in (1, 3, 4, 5)] +
    ["many rounds", "pattern extremes", "pattern nonfinite", "a NaN tap"])

#: (kernel, mode, n) of test_gpu_fir_runs.py::test_filter_and_reductions, and the seed each takes its taps from
EXISTING_SHAPES = (("t0", "s", 8192, 0), ("t0", "v", 1000, 8), ("t0", "f", 1024, 0), ("boxcar16", "s", 2048, 4), ("step", "v", 512, 0), ("step", "f", 64, 0),
                   ("one", "s", 256, 0), ("runs24", "s", 4096, 0), ("runs24", "v", 1024, 0), ("long512", "s", 2048, 0), ("long512", "v", 512, 0), ("long512", "f", 520, 0))


def existing_reach(taps, mode, n):
    """a row of the issue's table: (m, mp, steps, breakpoints, group sizes, output steps on the vector-store path)"""
    m = len(taps)
    t = breakpoints(taps)[0]
    return (m, mp(m), n_steps(mode, m, n), len(t), sorted({G for _, G in groups(t)}), sum(kind == "vector" for _, kind in steps_of(mode, m, n)))


# ------------------------------------------------------------------------------------------------------------------------------------
# taps and rows
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def taps_of(runs, family):
    """float32, read-only.  exact: the q-th 'v' run holds (-1)^q (1 + 37 q mod 1021), the first and the last of them 1023 and 1022 in
    magnitude; pedestal: uniform in +-[0.5, 1] with the same alternating signs (neighbours always differ), seeded by the layout"""
    nv = sum(k == "v" for k, _ in runs)
    if family == "exact":
        mag = 1.0 + (37 * np.arange(nv)) % 1021
        if nv:
            mag[0], mag[-1] = 1023, (1022 if nv > 1 else 1023)
    else:
        mag = np.random.default_rng([nv, sum(l for _, l in runs), 977]).uniform(0.5, 1.0, nv)
    vals, q, prev = [], 0, 0.0
    for kind, _ in runs:
        if kind == "v":
            prev = (-1.0) ** q * mag[q]
            q += 1
        elif kind == "0":
            prev = 0.0
        vals.append(prev)
    k = np.repeat(np.array(vals), [l for _, l in runs]).astype(np.float32)
    k.setflags(write=False)
    return k


def taps(c, family):
    k = taps_of(c.runs, family)
    if c.tap_nan:
        k = k.copy()
        k[c.m // 2] = np.nan
        k.setflags(write=False)
    return k


LARGE, SMALL = 200, 1  # the many-rounds case: 4 * 1023 * 512 < 2^24 becomes 200 * 1023 * 32 < 2^24 for its 32 taps


def _plateau_rows(c):
    """the extremes case (a boxcar of 8 equal taps): rows whose filtered maximum and minimum are plateaus of equal outputs at chosen
    places.  A block of 8 + L - 1 equal samples gives L equal outputs, the first at ``a`` where the block starts at sample a + start - 7"""
    n, P, st, m = c.n, c.P, c.start, c.m
    steps = steps_of(c.mode, m, n)
    vec = [g for g, (_, kind) in enumerate(steps) if kind == "vector"]
    assert len(vec) >= 2 and steps[vec[0] - 1][1] == "start" and steps[vec[-1] + 1][1] == "p"
    first_vec, second_vec, behind_vec = steps[vec[0]][0], steps[vec[1]][0], steps[vec[-1] + 1][0]
    sign = 1.0 if taps_of(c.runs, "exact")[0] > 0 else -1.0

    def row(max_at, min_at, length=12):
        x = np.zeros(n)
        for a, v in ((max_at, 4.0 * sign), (min_at, -4.0 * sign)):
            lo = a + st - (m - 1)
            assert lo >= 0 and lo + m - 1 + length <= n
            x[lo:lo + m - 1 + length] = v
        return x

    lane = first_vec + 8 * 9  # a lane's first output in a vector step
    rows = [row(lane - 5, lane + 8 * 20 - 6),          # plateaus across a lane's eight outputs
            row(second_vec - 5, second_vec + 300),     # the maximum across two 512-output steps, the minimum across a lane's
            row(first_vec - 6, behind_vec - 6),        # across the border between a cut step and a vector step, at either end
            row(behind_vec - 4, first_vec - 3),        # the same, the other extreme
            np.zeros(n)]                               # an all-equal output
    # an extreme at output 0 (a plateau that begins there) and one at output P - 1 alone
    x = np.zeros(n)
    x[0] = 4.0 * sign
    if c.mode == "v":
        x[m] = 4.0 * sign  # (the outputs 0 .. m hold one of the two each)
    tail = m - st if c.mode != "v" else m  # the samples the last output sums
    x[n - tail:] = -4.0 * sign
    x[n - tail - 1] = 1.0 * sign
    rows.append(x)
    return np.stack(rows)


@functools.lru_cache(maxsize=None)
def rows_of(case_id, family, n_rows=None, n_waves=None):
    """(rows, n) float32, read-only.  exact, 'std': seeded integers in [-4, 4]; from two rows on, row 1 is an impulse in the first sample,
    row 2 one in the last, row 3 a constant, row 4 zeros.  pedestal: every row 1000 + uniform(-1, 1).  'nonfinite': a NaN in the first
    sample, in the last, +inf in the first, in the last, -inf and +inf in one row, and a finite row.  'rounds' (``n_rows`` rows on
    ``n_waves`` wavefronts): the rows of the first round hold integers up to +-200, NaN rows and infinity rows among them, every later row
    -- the one that follows on the same wavefront -- integers in [-1, 1]"""
    c = by_id(case_id)
    R = c.rows if n_rows is None else n_rows
    rng = np.random.default_rng([int(case_id[:3]), c.n, int(family == "exact"), R])
    if family == "pedestal":
        x = (PEDESTAL + rng.uniform(-1, 1, (R, c.n))).astype(np.float32)
    elif c.pattern == "extremes":
        x = _plateau_rows(c).astype(np.float32)
    elif c.pattern == "rounds":
        x = rng.integers(-SMALL, SMALL + 1, (R, c.n)).astype(np.float32)
        x[:n_waves] = rng.integers(-LARGE, LARGE + 1, (n_waves, c.n))
        x[0:n_waves:7, 0] = LARGE  # (a first prefix sum that is not zero)
        x[3:n_waves:16, c.n // 2] = np.nan
        x[5:n_waves:16, 1] = np.inf
        x[6:n_waves:16, c.n - 1] = -np.inf
    else:
        x = rng.integers(-4, 5, (R, c.n)).astype(np.float32)
        if c.pattern == "nonfinite":
            x[0, 0] = np.nan
            x[1, -1] = np.nan
            x[2, 0] = np.inf
            x[3, -1] = np.inf
            x[4, [c.n // 3, c.n // 3 + 40]] = [-np.inf, np.inf]
        else:
            for r, fill in ((1, "first"), (2, "last"), (3, "const"), (4, "zero")):
                if r < R:
                    x[r] = {"const": 3.0}.get(fill, 0.0)
                    if fill == "first":
                        x[r, 0] = 4.0
                    elif fill == "last":
                        x[r, -1] = -3.0
    x.setflags(write=False)
    return x


def thresholds(case_id, family, n_rows):
    """a threshold per row for the walks: a half-integer (no filtered sample of the exact family equals it), seeded"""
    rng = np.random.default_rng([int(case_id[:3]), 5])
    thr = (rng.integers(1, 3000, n_rows) + 0.5).astype(np.float32)
    return thr if family == "exact" else (thr * np.float32(0.25)).astype(np.float32)


def convolve_rows(x, k, mode, dtype):
    k = np.asarray(k).astype(dtype)
    return np.stack([np.convolve(row.astype(dtype), k, mode=MODES[mode]) for row in x])


def expect_rows(x, k, mode):
    """(want, finite rows, oracle's): per row the int64 convolution where the row is finite (zeros elsewhere) and oracle.convolve_wf in
    float32 on all rows -- what decides NaNs, infinities and the finite outputs beside them"""
    fin = np.isfinite(x).all(axis=1)
    P = out_len(mode, len(k), x.shape[1])
    want = np.zeros((len(x), P), dtype=np.int64)
    if np.isfinite(k).all() and fin.any():
        want[fin] = convolve_rows(x[fin], k, mode, np.int64)
    with np.errstate(all="ignore"):
        conv, rc = oracle.convolve_wf(np.ascontiguousarray(x), k, mode, P)
    assert rc == 0
    return want, fin, conv


@functools.lru_cache(maxsize=None)
def expect(case_id, family, n_rows=None, n_waves=None):
    """exact: (int64 convolution, finite rows, oracle's float32 rows, the float32 rows every per-event value is the oracle's of);
    pedestal: (float64 convolution, all rows, None, None)"""
    c = by_id(case_id)
    x, k = rows_of(case_id, family, n_rows, n_waves), taps(c, family)
    if family == "pedestal":
        return convolve_rows(x, k, c.mode, np.float64), np.ones(len(x), dtype=bool), None, None
    want, fin, conv = expect_rows(x, k, c.mode)
    if c.tap_nan:
        fin = np.zeros(len(x), dtype=bool)
    y = np.where(fin[:, None], want.astype(np.float32), conv).astype(np.float32)
    for a in (want, fin, conv, y):
        a.setflags(write=False)
    return want, fin, conv, y


def walks_and_picks(c):
    """what goes along with min_max: a walk back from t_max, one forward from t_min, pick-offs at both ends of the output"""
    return ("t_max", "t_min"), (0, c.P - 1)


# ------------------------------------------------------------------------------------------------------------------------------------
# recipes
# ------------------------------------------------------------------------------------------------------------------------------------
def _taps_loader(file, path):
    if file != TAPS_FILE:
        return None
    family, case_id = path.split("/")
    return np.array(taps(by_id(case_id), family))


def register_taps_loader():
    from dspeed_amd import lgdo_io

    if _taps_loader not in lgdo_io.CONSTANT_LOADERS:
        lgdo_io.CONSTANT_LOADERS.append(_taps_loader)


def recipe(c, family, keep):
    """convolve_wf -> min_max -> time_point_thresh (the walk back from the maximum), the filtered waveform an output or not"""
    register_taps_loader()
    names = ["t_min", "t_max", "a_min", "a_max", "walk0"] + (["wf_f"] if keep else [])
    procs = {
        "wf_f": {"function": "convolve_wf", "module": M, "args": ["waveform", f"loadlh5('{TAPS_FILE}', '{family}/{c.id}')", f"'{c.mode}'", f"wf_f({c.P}, 'f')"]},
        "t_min, t_max, a_min, a_max": f"{M}.min_max(wf_f, t_min, t_max, a_min, a_max)",
        "walk0": f"{M}.time_point_thresh(wf_f, thr, t_max, 0, walk0)"}
    return {"outputs": names, "processors": procs}, names


# ------------------------------------------------------------------------------------------------------------------------------------
# the kernel in NumPy, step by step (test_fir_runs_cases_cpu.py)
# ------------------------------------------------------------------------------------------------------------------------------------
def model(x, k, mode, mut=None, prefix=np.float64):
    """dsp_fir_runs_kernel's sum path on the finite rows ``x``: the padded window of mp carried and 512 new prefix sums, groups read as
    ``win[r + G - 1 - k]``, the carry from step to step, vector steps and cut steps.  Returns the rows with a margin of 512 elements at
    either end (NaN where nothing was written): a store outside [0, P) shows there.

    ``mut``: one wrong neighbour of the kernel -- ("t", b, d): breakpoint b d taps later; ("s", gi): group gi's first element one off;
    ("drop", gi): group gi left out; ("short", "old" | "new"): the carried window without its first / last element; ("carry", g): step g's
    total not carried; ("vec", lo, hi): the vector-step predicate off by one; ("start", 1): start one off.
    ``prefix``: the type the prefix sums and the carry are held in"""
    x = np.asarray(x)
    R, n = x.shape
    m = len(k)
    t, w = table(k)
    t = t.copy()
    kind, arg = (mut[0], mut[1:]) if mut else (None, ())
    if kind == "t":
        t[arg[0]] += arg[1]
    grp = groups(t)
    p, st, MP, PMP = out_len(mode, m, n), start(mode, m) + (arg[0] if kind == "start" else 0), mp(m), pmp(m)
    steps = n_steps(mode, m, n)
    buf = np.zeros((R, PMP + PSTEP + 72))  # (+ what lies behind a wavefront's window: the next one's, or the block's spare round)
    out = np.full((R, p + 2 * STEP), np.nan)
    carry = np.zeros(R, dtype=prefix)
    j = np.arange(STEP)
    for g in range(steps):
        live = int(np.clip(n - g * STEP, 0, STEP))
        xs = np.zeros((R, STEP), dtype=prefix)
        xs[:, :live] = x[:, g * STEP:g * STEP + live]
        ps = (carry[:, None] + np.cumsum(xs, axis=1, dtype=prefix)).astype(prefix)
        buf[:, window_index(MP + j)] = ps
        if not (kind == "carry" and arg[0] == g):
            carry = ps[:, -1]
        acc = np.zeros((R, STEP))
        for gi, (bi, G) in enumerate(grp):
            if kind == "drop" and arg[0] == gi:
                continue
            s = MP - t[bi] - (G - 1) + (1 if kind == "s" and arg[0] == gi else 0)
            for q in range(G):
                acc += w[bi + q] * buf[:, window_index(j + s + (G - 1) - q)]  # lane l, output r: win[r + G - 1 - q] = element 8 l + s + r + G - 1 - q
        c = g * STEP - st + j
        if output_step_vector(g, st, p, *(arg if kind == "vec" else ())):
            out[:, STEP + c] = acc
        else:
            valid = (c >= 0) & (c < p)
            out[:, STEP + c[valid]] = acc[:, valid]
        lo, hi = (window_index(1) if mut == ("short", "old") else 0), (window_index(MP - 1) if mut == ("short", "new") else PMP)
        buf[:, lo:hi] = buf[:, PSTEP + lo:PSTEP + hi].copy()
    return out


def inside(out):
    return out[:, STEP:-STEP]


def mutations(c):
    """the wrong neighbours that must show on case ``c`` (a sum-path case), from its geometry"""
    t = table(taps_of(c.runs, "exact"))[0]
    grp = groups(t)
    steps = steps_of(c.mode, c.m, c.n)
    # (a group whose every read lies at or behind the row's total reads the same one element on: 'v' with m = n and the breakpoint at 0)
    muts = [("t", 0, 1), ("t", len(t) - 1, -1), ("start", 1)] + [("s", gi) for gi, (b, G) in enumerate(grp) if c.start + 1 - t[b + G - 1] < c.n]
    for gi in range(1, len(grp)):  # the later groups of a ramp longer than a group
        if grp[gi - 1][1] == GROUP and t[grp[gi][0]] == t[grp[gi][0] - 1] + 1:
            muts.append(("drop", gi))
    if len(steps) >= 2 and c.n > STEP:
        muts.append(("carry", 0))
        # the newest carried sum, P[512 g], is what output 512 g - start + t - 1 reads at breakpoint t
        if any(0 <= g * STEP - c.start + b - 1 < c.P for g in range(1, len(steps)) for b in t if b >= 1):
            muts.append(("short", "new"))
    if len(steps) >= 2 and c.m == mp(c.m) and t[-1] == c.m and 0 <= STEP - c.start < c.P and c.n > STEP:
        muts.append(("short", "old"))
    names = classes(c)
    if "vector predicate: one output short at the start" in names:
        muts.append(("vec", 1, 0))
    if "vector predicate: one output short at the end" in names:
        muts.append(("vec", 0, 1))
    return muts


def last_occurrence_min_max(y):
    """min_max with the second of two equal samples winning: (t_min, t_max)"""
    y = np.asarray(y)
    P = y.shape[1]
    return P - 1 - np.argmin(y[:, ::-1], axis=1), P - 1 - np.argmax(y[:, ::-1], axis=1)
