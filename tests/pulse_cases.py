"""The case book of the pulse picker (dsp_pulses.hip): rows, candidate lists, ratios and widths for ``peak_snr_threshold`` and
``multi_a_filter``, and an emulation of both written from their rules -- the yardstick of the GPU tests, itself held to what the reference's
bodies returned (tests/golden/pulses.npz, tools/gen_golden_pulses.py) by tests/test_pulse_cases_cpu.py.

A case is a block of rows of one length n with a list of m entries and a ratio each, and one width: ``named_cases`` holds the rows that
pin one rule each (their names say which), ``sweep_cases`` every (n, m, width) of the shapes at which the kernel takes another path.  Two
classes of rows have no reference result -- a candidate that is infinite or whose int() lies outside [0, n), and a zero sample at a
candidate --: ``EXEMPT`` names them, ``case["exempt"]`` marks them, and they are held to the emulation only.

Not a test module and not a conftest: a plain helper."""
import numpy as np

from dspeed_amd import _lib

BOOK = "pulses"
KERNEL = "dsp_pulses_kernel"
LOOPS = {"f32": np.float32, "f64": np.float64}
NAN, INF = float("nan"), float("inf")
LENGTHS = (2, 3, 21, 64, 65, 257, 1003)
LIST_LENGTHS = (1, 2, 20, 63, 64)
WIDTHS = (0, 1, 10, 64, "n")  # "n": as wide as the row, and wider
ROW_COUNTS = (1, 3, 4, 5, 9)  # rows that follow another on a wavefront's workgroup, and a workgroup partly empty
EXEMPT = ("outside-below", "outside-fraction-below", "outside-n", "outside-above", "plus-inf", "minus-inf", "zero-at-candidate", "zero-at-candidate-and-minimum")
#: the wrong neighbours of the rule that tests/test_pulse_cases_cpu.py holds the book against, one at a time
WRONG = ("window_includes_b", "last_tie", "b_clamped_to_n", "no_abs", "less_or_equal", "rounded_index", "nan_kept_in_place", "picker_row_nan_check",
         "no_pickoff_row_nan_check")


def width_of(width, n):
    return n + 5 if width == "n" else width


# ---------------------------------------------------------------------------------------------------------------- the emulation
def _min_index(w, a, b, last_tie=False):
    """the search ``for j in range(a, b): if w[j] < w[min_index]: min_index = j`` from min_index = a: the first of the lowest samples; a NaN
    never replaces the running minimum, and a NaN at a is never replaced (no comparison with it is true)"""
    if b <= a or np.isnan(w[a]):
        return a
    seg = np.where(np.isnan(w[a:b]), np.inf, w[a:b])
    if last_tie:
        return a + len(seg) - 1 - int(np.argmin(seg[::-1]))
    return a + int(np.argmin(seg))


def emulate_picker(rows, lists, ratio, width, T, wrong=()):
    """peak_snr_threshold on every row: (idx_out, n_idx_out, trace); ``trace[r, i]`` is the min_index of candidate i (-1: none looked for) --
    the order of tied minima shows nowhere else.  ``ratio``: one value or one per row.  ``wrong``: names of ``WRONG``, for the neighbours."""
    rows, lists = np.atleast_2d(np.asarray(rows)).astype(T), np.atleast_2d(np.asarray(lists, dtype=T))
    R, n = rows.shape
    m = lists.shape[1]
    ratio = np.broadcast_to(np.asarray(ratio, dtype=T), (R,))
    wd = int(width)
    out, count, trace = np.full((R, m), np.nan, T), np.zeros(R, np.uint32), np.full((R, m), -1, np.int64)
    with np.errstate(all="ignore"):
        for r in range(R):
            w, k = rows[r], 0
            if "picker_row_nan_check" in wrong and np.isnan(w).any():
                continue
            for i in range(m):
                idx = lists[r, i]
                if np.isnan(idx):
                    k += 1 if "nan_kept_in_place" in wrong else 0
                    continue
                if not (-1.0 < float(idx) < n):  # infinite, or int() outside the row: dropped, no sample read (the device's decision)
                    continue
                c = int(np.rint(idx)) if "rounded_index" in wrong else int(idx)  # int(): towards zero
                c = min(max(c, 0), n - 1)  # (the rounding neighbour may leave the row)
                a, b = max(c - wd, 0), min(c + wd, n if "b_clamped_to_n" in wrong else n - 1)
                if "window_includes_b" in wrong:
                    b = min(b + 1, n)
                lo = _min_index(w, a, b, "last_tie" in wrong)
                trace[r, i] = lo
                q = w[lo] / w[c]  # in the loop's type
                q = q if "no_abs" in wrong else np.abs(q)
                if (q <= ratio[r]) if "less_or_equal" in wrong else (q < ratio[r]):
                    out[r, k] = idx  # as given, not truncated
                    k += 1
            count[r] = k
    return out, count, trace


def emulate_pickoff(rows, lists, T, wrong=()):
    """multi_a_filter on every row: (va_max_out, fatal); ``fatal[r]``: the row holds a position that is no whole number, the reference's
    DSPFatal (its amplitudes are then nobody's: NaN here)"""
    rows, lists = np.atleast_2d(np.asarray(rows)).astype(T), np.atleast_2d(np.asarray(lists, dtype=T))
    R, n = rows.shape
    m = lists.shape[1]
    assert m < n, "The length of your return array must be smaller than the length of your waveform"
    out, fatal = np.full((R, m), np.nan, T), np.zeros(R, bool)
    for r in range(R):
        if np.isnan(rows[r]).any() and "no_pickoff_row_nan_check" not in wrong:
            continue
        for j in range(m):
            t = lists[r, j]
            if np.isnan(t) or t < 0 or t > n - 1:
                continue
            if int(t) != t:
                fatal[r] = True
                continue
            out[r, j] = rows[r, int(t)]
        if fatal[r]:
            out[r] = np.nan
    return out, fatal


# ---------------------------------------------------------------------------------------------------------------- the cases
def _case(key, names, rows, lists, ratio, width, T, exempt=()):
    rows, lists = np.asarray(rows, dtype=T), np.asarray(lists, dtype=T)
    assert rows.ndim == 2 and lists.ndim == 2 and len(rows) == len(lists) == len(ratio) == len(names)
    return {"key": key, "names": list(names), "rows": rows, "lists": lists, "ratio": np.asarray(ratio, dtype=T), "width": int(width),
            "n": rows.shape[1], "m": lists.shape[1], "exempt": np.array([nm in exempt for nm in names])}


N0 = 21  # the rows of the named cases


def _flat(level=50.0, **at):
    """a row of N0 samples at ``level``, with the samples named: _flat(c10=100, c13=1)"""
    w = np.full(N0, level)
    for k, v in at.items():
        w[int(k[1:])] = v
    return w


def named_cases(loop):
    """every named case of the issue, four candidates a list; grouped by width"""
    T = LOOPS[loop]
    groups = {}

    def add(width, name, row, cands, ratio):
        cands = list(cands) + [NAN] * (4 - len(cands))
        groups.setdefault(width, []).append((name, row, cands[:4], ratio))

    # ---- the window (candidate 10 of a flat row at 50 with 100 at the candidate: a quotient of 0.5 unless a lower sample is seen)
    add(3, "minimum-at-c-plus-width-unseen", _flat(c10=100, c13=1), [10], 0.3)       # b = 13 is never looked at: 0.5, dropped
    add(3, "minimum-at-c-plus-width-minus-1-seen", _flat(c10=100, c12=1), [10], 0.3)  # ... 12 is: kept
    add(5, "minimum-at-last-sample-unseen-under-the-clamp", _flat(c18=100, c20=1), [18], 0.3)  # b = min(23, 20) = 20: unseen
    add(5, "minimum-at-last-but-one-seen-under-the-clamp", _flat(c18=100, c19=1), [18], 0.3)
    add(3, "minimum-at-a", _flat(c10=100, c7=1), [10], 0.3)
    add(3, "minimum-just-below-a-unseen", _flat(c10=100, c6=1), [10], 0.3)
    add(3, "tied-minima", _flat(c10=100, c8=5, c11=5, c12=5), [10], 0.3)
    add(3, "tied-minima-of-zero-signs", _flat(c10=100, c8=-0.0, c11=0.0), [10], 0.3)
    add(5, "window-clamped-at-0", _flat(c2=100, c0=1), [2], 0.3)
    add(5, "candidate-0-and-n-1", _flat(c0=100, c1=1, c20=100, c19=1), [0, 20], 0.3)
    add(0, "width-0-ratio-above-1", _flat(c10=100), [10, 3], 1.5)   # an empty window: the quotient is 1
    add(0, "width-0-ratio-below-1", _flat(c10=100), [10, 3], 0.5)
    add(0, "width-0-ratio-1-strict", _flat(c10=100), [10, 3], 1.0)
    add(N0 + 5, "width-wider-than-the-row", _flat(c10=100, c0=1, c20=0.5), [10, 0, 20], 0.3)  # [0, 20): sample 20 unseen
    # ---- the row
    add(3, "negative-minimum-abs-matters", _flat(c10=100, c9=-50), [10], 0.3)  # |-0.5| = 0.5: dropped; -0.5 < 0.3 would keep it
    add(3, "negative-candidate-sample", _flat(level=-50.0, c10=-40), [10], 1.1)  # the minimum is -50: |(-50) / (-40)| = 1.25, dropped
    add(3, "all-negative-kept", _flat(level=-50.0, c10=-40), [10], 1.3)
    add(3, "plus-inf-at-candidate", _flat(c10=INF), [10, 4], 0.3)              # x / inf = 0: kept; candidate 4: quotient 1
    add(3, "minus-inf-in-window", _flat(c10=100, c9=-INF), [10], 0.3)           # |-inf / 100| = inf: dropped
    add(3, "minus-inf-over-plus-inf", _flat(c10=INF, c9=-INF), [10], 0.3)       # NaN: dropped
    add(3, "nan-inside-window", _flat(c10=100, c9=NAN, c11=1), [10], 0.3)       # the NaN never takes the minimum: 1 / 100, kept
    add(3, "nan-at-window-start", _flat(c10=100, c7=NAN, c11=1), [10], 0.3)     # min_index = a holds a NaN and keeps it: dropped
    add(3, "nan-at-candidate", _flat(c10=NAN, c11=1), [10, 3], 0.3)             # x / NaN: dropped; candidate 3 sees no NaN
    add(3, "nan-outside-every-window", _flat(c10=100, c11=1, c20=NAN), [10, 3], 0.3)  # the picker does not look; the pick-off gives NaNs
    # ---- the list
    add(3, "all-nan", _flat(c10=100, c11=1), [NAN, NAN, NAN, NAN], 0.3)
    add(3, "nans-in-front", _flat(c10=100, c11=1), [NAN, NAN, 10, 10], 0.3)
    add(3, "nans-in-the-middle", _flat(c10=100, c11=1, c3=100, c4=1), [10, NAN, NAN, 3], 0.3)
    add(3, "nans-trailing", _flat(c10=100, c11=1), [10, NAN, NAN, NAN], 0.3)
    add(3, "duplicates", _flat(c10=100, c11=1), [10, 10, 10, 10], 0.3)
    add(3, "unsorted", _flat(c10=100, c11=1, c3=100, c4=1, c17=100), [17, 10, 3, 10], 0.3)
    add(3, "half-integer-kept", _flat(c10=100, c11=1, c9=70), [10.5], 0.3)      # int() = 10; rounded (to even): 10 as well
    add(3, "half-integer-truncated-not-rounded", _flat(c11=100, c12=70, c10=1), [11.5], 0.012)  # int() = 11: 1 / 100 kept; at 12: 1 / 70, dropped
    add(3, "fraction-truncated-not-rounded", _flat(c10=100, c11=70, c9=1), [10.75], 0.012)  # int() = 10: 1 / 100 kept; at 11: 1 / 70, dropped
    add(1, "fraction-in-minus-1-0", _flat(c0=100, c1=70), [-0.5, -0.25, -0.999], 0.8)  # int() = 0, the window [0, 1): quotient 1, dropped
    add(1, "fraction-in-minus-1-0-kept", _flat(c0=100, c1=70), [-0.5, -0.0, -0.999], 1.5)  # kept as given: the pick-off gives NaN, w[0], NaN
    add(3, "every-candidate-kept", _flat(c10=100, c11=1, c3=100, c4=1, c16=100, c17=1, c7=2), [3, 10, 16, 10], 0.3)
    add(3, "none-kept", _flat(c10=100, c3=100, c16=100), [3, 10, 16, 10], 0.3)
    add(3, "kept-and-dropped-alternate", _flat(c10=100, c11=1, c3=100, c16=100, c17=1, c1=100), [3, 10, 1, 16], 0.3)
    # ---- the ratio
    add(3, "nan-ratio", _flat(c10=100, c11=1), [10, 10], NAN)
    add(3, "ratio-equal-to-the-quotient", _flat(c10=100), [10, 3], 0.5)          # 50 / 100 < 0.5 is false
    add(3, "ratio-just-above-the-quotient", _flat(c10=100), [10, 3], float(np.nextafter(T(0.5), T(1))))
    add(3, "ratio-zero-and-negative", _flat(c10=100, c11=0.0, c9=-0.0), [10], 0.0)  # |0 / 100| < 0 is false
    add(3, "ratio-inf", _flat(c10=100, c3=7), [10, 3, 5], INF)
    # ---- where the reference defines nothing (EXEMPT): held to the emulation only
    add(3, "outside-below", _flat(c10=100, c11=1), [-1, 10, -7], 0.3)
    add(3, "outside-fraction-below", _flat(c10=100, c11=1), [-1.5, 10, -1.0], 0.3)
    add(3, "outside-n", _flat(c10=100, c11=1), [N0, 10], 0.3)
    add(3, "outside-above", _flat(c10=100, c11=1), [N0 + 0.5, 1e9, 10, 3e38], 0.3)
    add(3, "plus-inf", _flat(c10=100, c11=1), [INF, 10], 0.3)
    add(3, "minus-inf", _flat(c10=100, c11=1), [10, -INF], 0.3)
    add(3, "zero-at-candidate", _flat(c10=0.0), [10, 3], 0.3)                    # 50 / 0 = inf: dropped
    add(3, "zero-at-candidate-and-minimum", _flat(c10=0.0, c9=0.0, c3=-0.0, c4=-5), [10, 3], 0.3)  # 0 / 0 = NaN: dropped
    return [_case(f"named_{loop}_w{width}", [g[0] for g in group], [g[1] for g in group], [g[2] for g in group], [g[3] for g in group], width, T, EXEMPT)
            for width, group in sorted(groups.items())]


SWEEP_ROWS = ("pulses", "noise", "negative", "steps", "one-nan", "row-ratio")


def sweep_cases(loop):
    """every length, list length and width: a pulse train on noise, noise alone, a negative row, integer steps with many ties, a row with one
    NaN, and the pulses again under a ratio that differs per row; the candidates are places of the row, pulses at every other one, NaNs among them"""
    T = LOOPS[loop]
    cases = []
    for n in LENGTHS:
        for m in LIST_LENGTHS:
            for width in WIDTHS:
                rng = np.random.default_rng([n, m, width_of(width, n)])
                t = np.arange(n)
                places = np.sort(rng.choice(n, size=min(m, n), replace=False)) if n > 1 else np.zeros(1, int)
                pulses = rng.normal(0, 1, n) + 20
                for p in places[::2]:
                    pulses += 200 * np.exp(-0.5 * ((t - p) / 1.5) ** 2) - 60 * np.exp(-0.5 * ((t - p - 4) / 2.0) ** 2)
                steps = np.floor(t / 3) % 5 - 2.0
                steps[steps == 0] = 1.0  # (no zero sample: that class is EXEMPT)
                one_nan = pulses.copy()
                one_nan[int(rng.integers(n))] = np.nan
                rows = [pulses, rng.normal(0, 1, n) + 5, -pulses, steps, one_nan, pulses]
                lists = []
                for k in range(len(rows)):
                    c = np.full(m, np.nan)
                    pick = rng.choice(places, size=min(m, len(places)), replace=(k == 3))
                    c[:len(pick)] = np.sort(pick) if k != 3 else pick
                    if m > 2:
                        c[rng.integers(m, size=max(1, m // 6))] = np.nan  # NaNs anywhere, trailing ones where the list is longer than the row
                    lists.append(c)
                ratio = [0.8, 0.9, 0.8, 0.75, 0.8, float(rng.uniform(0.2, 1.2))]
                cases.append(_case(f"sweep_{loop}_n{n}_m{m}_w{width}", SWEEP_ROWS, rows, lists, ratio, width_of(width, n), T))
    return cases


def all_cases(loop):
    return named_cases(loop) + sweep_cases(loop)


def tile_rows(a, count):
    """``count`` rows: those of ``a``, over and over"""
    a = np.asarray(a)
    return a[np.arange(count) % len(a)]


def integer_rows(rows, rows_type):
    """the rows as an integer type holds them: whole numbers in its range; a NaN or an infinity has no integer, those samples become 1"""
    w = np.where(np.isfinite(rows), np.rint(rows), 1)
    w = np.abs(w) if np.dtype(rows_type).kind == "u" else w
    return w.astype(rows_type)


# ---------------------------------------------------------------------------------------------------------------- programs
def program(n, m=20, rows=np.float32, loop=np.float32, pick=True, amp=False, store_list=True, ratio=0.8, width=10.0, offset=0, row_stride=None,
            list_offset=0, list_stride=None, out_stride=None, out_len=None, amp_len=None, count_type=np.uint32):
    """LOAD, LOAD of the list, [PEAK_SNR_THRESHOLD,] [MULTI_A_FILTER,] [STORE of idx_out,] [STORE of va_max_out,] [STORE_SCALAR]; ``ratio`` /
    ``width``: a number, or "column" for a per-event binding"""
    from dspeed_amd.chain import Program, Scalar

    p = Program()
    s_in, s_list = p.add_slot(n), p.add_slot(m)
    p.add_op(_lib.OP_LOAD, dst=s_in, io=p.add_io("w", _lib.IO_WF_IN, rows, n, offset, row_stride))
    p.add_op(_lib.OP_LOAD, dst=s_list, io=p.add_io("list", _lib.IO_WF_IN, loop, m, list_offset, list_stride))
    src_list = s_list
    operand = lambda v, name: Scalar.input(p.add_io(name, _lib.IO_SCALAR_IN, loop)) if v == "column" else Scalar.const(v)  # noqa: E731
    if pick:
        s_idx = p.add_slot(m if out_len is None else out_len)
        reg = p.add_sregs(1)
        p.add_op(_lib.OP_PEAK_SNR_THRESHOLD, dst=s_idx, src=s_in, ip=(s_list, reg), sp=(operand(ratio, "ratio"), operand(width, "width")))
        src_list = s_idx
    if amp:
        s_amp = p.add_slot(p.slots[src_list] if amp_len is None else amp_len)
        p.add_op(_lib.OP_MULTI_A_FILTER, dst=s_amp, src=s_in, ip=(src_list,))
    if pick and store_list:
        p.add_op(_lib.OP_STORE, src=s_idx, io=p.add_io("idx_out", _lib.IO_WF_OUT, loop, p.slots[s_idx], 0, out_stride))
    if amp:
        p.add_op(_lib.OP_STORE, src=s_amp, io=p.add_io("va_max", _lib.IO_WF_OUT, loop, p.slots[s_amp], 0, out_stride))
    if pick:
        p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io("count", _lib.IO_SCALAR_OUT, count_type), ip=(reg,))
    return p
