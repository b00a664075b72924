"""Is the case list of fir_runs_cases.py what it claims?  On the planner, the oracle and NumPy alone (no device): the geometry is the
kernel's; every class of step, window, group and table geometry is hit by a case that names it; what test_gpu_fir_runs.py's own twelve
shapes reach is the incomplete set the list was made for; a NumPy model of the kernel, step by step, equals the int64 convolution on every
exact case, and each of its wrong neighbours changes the expectation of every case of the class it belongs to; the extremes rows tell a
last-occurrence min_max from the oracle's; the pedestal family leaves float64 prefix sums half of the bar and float32 ones none of it;
and the planner refuses the neighbours it should.  If a changed rule breaks a condition here, the rule (or the input) is what changes,
never the bar."""
import os

import numpy as np
import pytest

import fir_runs_cases as K
import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "dspeed_amd", "csrc")
CASES = K.cases()
IDS = [c.id for c in CASES]
SUM_IDS = [c.id for c in CASES if c.sum_path and c.pattern != "rounds"]
ROUNDS = dict(n_rows=41, n_waves=20)  # the many-rounds case here: two rounds and a row on 20 wavefronts (the device test asks the chain)


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _finite_exact(case_id):
    c = K.by_id(case_id)
    kw = ROUNDS if c.pattern == "rounds" else {}
    want, fin, conv, y = K.expect(case_id, "exact", **kw)
    return c, K.rows_of(case_id, "exact", **kw)[fin].astype(np.float64), K.taps(c, "exact"), want[fin]


# ------------------------------------------------------------------------------------------------------------------------------------
# the geometry and the classes
# ------------------------------------------------------------------------------------------------------------------------------------
def test_the_constants_and_formulas_are_the_kernels():
    h, k, plan, prog = _source("dsp_kernels.h"), _source("dsp_fir_runs.hip"), _source("dsp_plan.cpp"), _source("dsp_program.h")
    assert f"constexpr int STEP = {K.STEP};" in h and "return (4 * (mp + mp / 8 + STEP + STEP / 8) + 64) * (int)sizeof(double);" in h
    assert f"#define DSP_FIR_RUNS_MAX {K.RUNS_MAX} " in prog and f"#define DSP_FIR_RUNS_MAX_TAPS {K.MAX_TAPS}" in prog and f"#define DSP_FIR_RUNS_GROUP {K.GROUP} " in prog
    assert "const int mp = (m + 63) & ~63;" in k and "constexpr int PSTEP = STEP + STEP / 8;" in k and "const int pmp = mp + mp / 8;" in k
    assert "const int n_steps = (p + start + STEP - 1) / STEP;" in k and "if (g * STEP + STEP <= n) {" in k
    assert "if (g * STEP - start >= 0 && g * STEP - start + STEP <= p) {" in k and "win[j] = row9[q + (q >> 3)];" in k
    assert "const int s = mp - __builtin_amdgcn_readlane(tab_t, bi) - (G - 1);" in k and "win[r + (G - 1) - k]" in k
    assert "const bool ok = !(bad || n_break > DSP_FIR_RUNS_MAX + 1);" in k
    assert "A.start = mode == 'v' ? m - 1 : (mode == 's' ? (m - 1) / 2 : 0);" in plan and "if (!A.keep) A.out_stride = (P + 63) & ~63;" in plan
    assert "if (m < 1 || m > n || m > DSP_FIR_RUNS_MAX_TAPS) return false;" in plan
    assert K.lds_bytes(512) == (4 * (576 + 576) + 64) * 8 <= 160 * 1024 // 4 and K.lds_bytes(1) == (4 * (72 + 576) + 64) * 8
    assert K.window_index(np.arange(16)).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16] and K.scratch_pitch(513) == 576
    # start is where 'valid' and 'same' begin in the full convolution
    x, rng = np.arange(1.0, 25.0), np.random.default_rng(0)
    for m in (1, 2, 7, 8, 24):
        k = rng.integers(1, 9, m).astype(np.float64)
        full = np.convolve(x, k, "full")
        for mode in "vsf":
            assert np.array_equal(np.convolve(x, k, K.MODES[mode]), full[K.start(mode, m):K.start(mode, m) + K.out_len(mode, m, len(x))])


def test_breakpoints_and_groups_on_known_kernels():
    import golden_util

    t, w, raw, finite = K.breakpoints(golden_util.recipe_kernel("t0"))
    assert raw == 10 and finite and t.tolist() == list(range(9)) + [133] and K.groups(t) == [(0, 8), (8, 1), (9, 1)] and K.ramps(t) == [9, 1]
    assert abs(w.sum()) < 1e-12  # (the weights are differences: they telescope from zero to zero)
    t, w, raw, finite = K.breakpoints(np.float32([0, 0, 2, 2, -0.0, 0.0, 3]))
    assert t.tolist() == [2, 4, 6, 7] and w.tolist() == [2, -2, 3, -3]
    assert K.breakpoints(np.float32([1, np.nan, 1]))[2:] == (4, False) and K.breakpoints(np.float32([1, np.inf]))[3] is False
    assert K.table(np.zeros(5, np.float32)) is None and K.table(np.float32([1, np.nan])) is None
    assert K.table(np.arange(1, 25, dtype=np.float32)) is not None and K.table(np.arange(1, 26, dtype=np.float32)) is None  # 25 and 26 breakpoints
    assert K.groups(np.arange(17)) == [(0, 8), (8, 8), (16, 1)] and K.groups(np.array([0, 2, 3, 9])) == [(0, 1), (1, 2), (3, 1)]


def test_every_class_is_hit_by_a_case_that_names_it():
    hit = {}
    for c in CASES:
        cl = K.classes(c)
        assert c.why in cl, (c.id, c.why, cl)
        for name in cl:
            hit.setdefault(name, []).append(c)
    assert not [name for name in K.CLASSES if name not in hit]
    assert len(IDS) == len(set(IDS))
    # every group size in every position on the sum path, with the kept output and the reductions in both families
    for G in range(1, 9):
        for pos in ("front", "end", "middle"):
            assert any(c.sum_path and "pedestal" in c.families for c in hit[f"G={G} {pos}"])
    # both guarded tails of the three-buffer rotation and a full turn: n_steps = 1 .. 7 hold every residue mod 3 twice
    assert {K.n_steps(c.mode, c.m, c.n) for c in CASES} >= set(range(1, 8))
    for c in CASES:  # "64 live lanes" is the full-step branch of the last input step, anything less the guarded one
        last = (c.n - 1) // K.STEP
        assert K.input_step_full(last, c.n) == ("last input step 64 live lanes" in K.classes(c)) and not K.input_step_full(last + 1, c.n)
    # the sizes stay small
    assert max(c.n for c in CASES) == 3080 and max(c.rows for c in CASES) == 6 and len(CASES) < 140
    assert sum(c.recipe for c in CASES) >= 10
    rec = [c for c in CASES if c.recipe]
    assert any(not c.sum_path for c in rec) and any(c.m >= 64 for c in rec) and any(c.m < 64 for c in rec)


def test_the_existing_shapes_reach_what_the_issue_says():
    """the premise: the twelve shapes of test_gpu_fir_runs.py never run group_of<3> .. group_of<7>, no ramp beyond 9 breakpoints, no table
    beyond 23 entries, m == mp only at 512, and a kept output at offset 0 alone"""
    import test_gpu_fir_runs as T

    marks = [m for m in T.test_filter_and_reductions.pytestmark if m.name == "parametrize"][0].args[1]
    assert [(w, mode, n, off) for w, mode, n, off, _ in marks] == list(K.EXISTING_SHAPES)
    table = {("t0", "s"): (133, 192, 17, 10, [1, 8], 15), ("t0", "v"): (133, 192, 2, 10, [1, 8], 0), ("t0", "f"): (133, 192, 3, 10, [1, 8], 2),
             ("boxcar16", "s"): (16, 64, 5, 2, [1], 3), ("step", "v"): (12, 64, 1, 3, [1], 0), ("step", "f"): (12, 64, 1, 3, [1], 0),
             ("one", "s"): (1, 64, 1, 2, [2], 0), ("runs24", "s"): (232, 256, 9, 23, [1, 2], 7), ("runs24", "v"): (315, 320, 2, 23, [1, 2], 1),
             ("long512", "s"): (512, 512, 5, 5, [1], 3), ("long512", "v"): (512, 512, 1, 5, [1], 0), ("long512", "f"): (512, 512, 3, 5, [1], 2)}
    sizes, ms = set(), set()
    for which, mode, n, off in K.EXISTING_SHAPES:
        taps = T._taps(which, np.random.default_rng(n + off + len(which)))
        reach = K.existing_reach(taps, mode, n)
        assert reach == table[(which, mode)], (which, mode, reach)
        sizes |= set(reach[4])
        ms.add((reach[0], reach[1]))
        assert max(K.ramps(K.breakpoints(taps)[0])) <= 9
    assert sizes == {1, 2, 8} and {m for m, mp in ms if m == mp} == {512}
    assert K.breakpoints(np.random.default_rng(11).uniform(-1, 1, 40).astype(np.float32))[2] == 41  # (the first refused count the suite meets)


# ------------------------------------------------------------------------------------------------------------------------------------
# the two families
# ------------------------------------------------------------------------------------------------------------------------------------
def test_the_taps_are_what_the_families_say():
    for c in CASES:
        runs = c.runs
        k = K.taps_of(runs, "exact")
        vals = [k[i] for i in np.cumsum([0] + [l for _, l in runs])[:-1]]
        own = [v for v, (kind, _) in zip(vals, runs) if kind == "v"]
        assert k.dtype == np.float32 and len(k) == c.m and np.array_equal(k, np.rint(k)) and np.abs(k).max() <= 1023
        assert len(set(np.abs(own))) == len(own) and all(np.sign(v) == (-1) ** q for q, v in enumerate(own))
        if own:
            assert abs(own[0]) == 1023 and sorted(np.abs(own))[-2:] == ([1022, 1023] if len(own) > 1 else [1023])
        f = K.taps_of(runs, "pedestal")
        nz = f[f != 0]
        assert f.dtype == np.float32 and (np.abs(nz) >= 0.5).all() and (np.abs(nz) <= 1).all() and np.array_equal(f == 0, k == 0)
        # the same breakpoints in both families: the layout is the case
        assert np.array_equal(K.breakpoints(f)[0], K.breakpoints(k)[0])
    nan = next(c for c in CASES if c.tap_nan)
    assert np.isnan(K.taps(nan, "exact")).sum() == 1 and K.table(K.taps(nan, "exact")) is None


@pytest.mark.parametrize("case_id", IDS)
def test_the_rows_are_what_the_families_say(case_id):
    c = K.by_id(case_id)
    kw = ROUNDS if c.pattern == "rounds" else {}
    x = K.rows_of(case_id, "exact", **kw)
    want, fin, conv, y = K.expect(case_id, "exact", **kw)
    assert x.dtype == np.float32 and x.shape == ((c.rows or ROUNDS["n_rows"]), c.n) and y.shape == (len(x), c.P) and y.dtype == np.float32
    xf = x[np.isfinite(x).all(axis=1)]
    bound = K.LARGE if c.pattern == "rounds" else 4
    assert np.array_equal(xf, np.rint(xf)) and np.abs(xf).max() <= bound
    # every partial sum, in any order, is an integer below 2^24: the sum path and the tap-by-tap path are both exact
    assert bound * np.abs(K.taps_of(c.runs, "exact")).astype(np.float64).sum() < 2 ** 24 and np.abs(want).max() < 2 ** 24
    if not c.tap_nan:
        assert np.array_equal(conv[fin].astype(np.int64), want[fin]) and np.array_equal(y[fin], want[fin])
    if c.pattern == "std":
        assert np.isfinite(x).all() and (fin.all() or c.tap_nan)
        if c.rows >= 5:
            assert np.count_nonzero(x[1]) == 1 and x[1, 0] != 0 and np.count_nonzero(x[2]) == 1 and x[2, -1] != 0 and (x[3] == 3).all() and not x[4].any()
    elif c.pattern == "nonfinite":
        assert np.isnan(x[0, 0]) and np.isnan(x[1, -1]) and x[2, 0] == np.inf and x[3, -1] == np.inf and set(x[4][np.isinf(x[4])]) == {-np.inf, np.inf}
        assert fin.tolist() == [False] * 5 + [True] and np.isnan(y[:2]).all()
        for r in (2, 3, 4):  # an infinity leaves the outputs it does not meet finite, and they are the integers of the convolution without it
            ok = np.isfinite(y[r])
            assert ok.any() and not ok.all()
            clean = np.where(np.isfinite(x[r]), x[r], 0).astype(np.int64)
            assert np.array_equal(y[r][ok], np.convolve(clean, K.taps(c, "exact").astype(np.int64), K.MODES[c.mode])[ok])
        if any(kind == "0" for kind, _ in c.runs):
            assert np.isnan(y[2]).any()  # (an infinity under a zero tap)
    elif c.pattern == "rounds":
        nw = ROUNDS["n_waves"]
        assert np.abs(xf[:4]).max() > 100 and np.abs(x[nw:]).max() <= K.SMALL and fin[nw:].all() and not fin[3] and not fin[5] and not fin[6]
    if c.tap_nan:
        assert np.isnan(y).all() and not fin.any()
    for family in c.families[1:]:
        xp = K.rows_of(case_id, family, **kw)
        assert xp.dtype == np.float32 and np.abs(xp - xp.mean()).max() <= 500 and xp.min() > 998
        frac = np.abs(xp.astype(np.float64)) * 2.0 ** 14  # 1000 + u: the last of 24 bits is worth 2^-14
        assert (np.rint(frac) == frac).all() and (frac % 2 == 1).mean() > 0.4  # (full significands: the last bit is set in half of them)


@pytest.mark.parametrize("case_id", [c.id for c in CASES if c.sum_path])
def test_the_model_of_the_kernel_equals_the_int64_convolution(case_id):
    c, x, k, want = _finite_exact(case_id)
    out = K.model(x, k, c.mode)
    assert np.array_equal(K.inside(out), want.astype(np.float64))
    assert np.isnan(out[:, :K.STEP]).all() and np.isnan(out[:, -K.STEP:]).all()  # nothing stored outside [0, P)


@pytest.mark.parametrize("case_id", SUM_IDS)
def test_every_wrong_neighbour_of_the_model_changes_the_expectation(case_id):
    """a breakpoint one tap off, a group's first element one off, a later group of a long ramp dropped, the carried window one element
    short at either end, a step's total not carried, the vector-step predicate one output wide at either end, start one off: on every case
    of the class each belongs to (``fir_runs_cases.mutations`` says which, from the geometry)"""
    c, x, k, want = _finite_exact(case_id)
    right = K.model(x, k, c.mode)
    muts = K.mutations(c)
    assert {("t", 0, 1), ("start", 1)} <= set(muts) and len([m for m in muts if m[0] == "s"]) >= len(K.groups(K.table(k)[0])) - 1
    for mut in muts:
        assert not np.array_equal(K.model(x, k, c.mode, mut=mut), right, equal_nan=True), mut


def test_the_wrong_neighbours_cover_their_classes():
    by_kind = {}
    for c in CASES:
        if c.sum_path and c.pattern != "rounds":
            for mut in K.mutations(c):
                by_kind.setdefault(mut[0] if mut[0] not in ("short", "vec") else mut, []).append(c)
    names = lambda c: K.classes(c)  # noqa: E731
    assert {"t", "s", "start", "carry", "drop", ("short", "new"), ("short", "old"), ("vec", 1, 0), ("vec", 0, 1)} == set(by_kind)
    assert {L for c in by_kind["drop"] for L in (9, 16, 17) if f"ramp {L}" in names(c)} == {9, 16, 17}
    assert all(K.n_steps(c.mode, c.m, c.n) >= 2 for c in by_kind["carry"]) and len(by_kind["carry"]) > 50
    assert all("m == mp: the last breakpoint reads window element 0" in names(c) for c in by_kind[("short", "old")])
    assert {c.m for c in by_kind[("short", "old")]} >= {64, 128, 512}
    # the predicate's wrong neighbours store outside the row: the margins of the model's rows catch them, the sentinels of the device's
    for mut in (("vec", 1, 0), ("vec", 0, 1)):
        for c in by_kind[mut]:
            _, x, k, want = _finite_exact(c.id)
            out = K.model(x, k, c.mode, mut=mut)
            assert np.array_equal(K.inside(out), want.astype(np.float64)) and not np.isnan(out[:, K.STEP - 1] if mut[1] else out[:, -K.STEP]).any()
    assert any(c.off for c in by_kind[("vec", 1, 0)])


def test_the_extremes_rows_tell_first_from_last_occurrence():
    seen = []
    for c in CASES:
        if c.pattern != "extremes":
            continue
        seen.append(c.mode)
        want, fin, conv, y = K.expect(c.id, "exact")
        t_min, t_max, a_min, a_max, rc = oracle.min_max(np.ascontiguousarray(y))
        assert rc == 0 and fin.all()
        l_min, l_max = K.last_occurrence_min_max(y)
        assert ((l_min != t_min) | (l_max != t_max)).all()
        steps = K.steps_of(c.mode, c.m, c.n)
        edges = [c0 for c0, _ in steps[1:]]
        assert [kind for _, kind in steps] == ["start", "vector", "vector", "p"]

        def crosses(first, last, where):
            return first < where <= last

        lane = lambda t: (int(t) - edges[0]) // 8  # noqa: E731
        # row 0: both plateaus across a lane's eight outputs inside a vector step; row 1: the maximum across two vector steps
        assert lane(t_max[0]) != lane(l_max[0]) and lane(t_min[0]) != lane(l_min[0]) and edges[0] < t_max[0] and l_min[0] < edges[1]
        assert crosses(t_max[1], l_max[1], edges[1])
        # rows 2 and 3: each extreme across cut -> vector and across vector -> cut
        assert crosses(t_max[2], l_max[2], edges[0]) and crosses(t_min[2], l_min[2], edges[2])
        assert crosses(t_min[3], l_min[3], edges[0]) and crosses(t_max[3], l_max[3], edges[2])
        # row 4: all equal; row 5: the maximum a plateau from output 0, the minimum at output P - 1 alone
        assert (y[4] == y[4, 0]).all() and t_min[4] == t_max[4] == 0
        assert t_max[5] == 0 and l_max[5] > 0 and t_min[5] == c.P - 1 == l_min[5]
    assert sorted(seen) == ["s", "v"]


@pytest.mark.parametrize("case_id", [c.id for c in CASES if "pedestal" in c.families])
def test_pedestal_family_leaves_float64_sums_half_of_the_bar_and_float32_sums_none(case_id):
    """The kernel's arithmetic with float64 prefix sums, rounded to float32 as the kernel stores it, stays below TOL / 2 of the filtered
    peak on every row: a condition on the inputs (a case whose taps cancelled the pedestal would fail here, and gets other taps).  With
    the prefix sums and the carry in float32 the same model misses the bar: a cumulative sum of n samples near 1000 is rounded to 2^-24
    of 1000 n at every step, against a peak of 1000 |sum of the taps under the window|.  That holds by a margin where the row is long and
    the kernel short, n >= 504 and m <= 65, and is asserted there; the other cases' figures are printed"""
    c = K.by_id(case_id)
    kw = ROUNDS if c.pattern == "rounds" else {}
    x, k = K.rows_of(case_id, "pedestal", **kw), K.taps(c, "pedestal")
    want = K.expect(case_id, "pedestal", **kw)[0]
    peak = np.abs(want).max(axis=1, keepdims=True)
    assert (peak > 500).all()
    e64 = np.abs(K.inside(K.model(x.astype(np.float64), k, c.mode)).astype(np.float32) - want) / peak
    e32 = np.abs(K.inside(K.model(x, k, c.mode, prefix=np.float32)) - want) / peak
    print(f"FIGURE {case_id}: float64 sums {e64.max():.3e}, float32 sums {e32.max():.3e} of the peak")
    assert e64.max() <= 0.5 * K.TOL
    if c.n >= 504 and c.m <= 65:
        assert e32.max(axis=1).min() > K.TOL


# ------------------------------------------------------------------------------------------------------------------------------------
# the planner and the compiler
# ------------------------------------------------------------------------------------------------------------------------------------
def _plan_of(c, **kw):
    import test_gpu_fir_runs as T
    from dspeed_amd.chain import plan

    walk_from, picks = K.walks_and_picks(c)
    prog, _, _ = T._program(c.n, 0, c.n, K.taps(c, "exact"), c.mode, walk_from=walk_from, picks=picks, out_offset=c.off, out_stride=c.stride, **kw)
    return plan(prog)


def test_every_case_plans_onto_the_kernel_kept_and_unkept():
    for c in CASES:
        for keep in (True, False):
            p = _plan_of(c, keep=keep)
            assert p["kernel"] == "dsp_fir_runs_kernel", (c.id, keep, p["kernel"], p["note"])
        assert K.admitted(c.n, c.m, c.mode)


def test_the_planner_refuses_the_neighbours():
    """n = 60 and n % 8 = 4, m = n + 1, m = 513, a row offset or stride that is no multiple of 4 elements, int16 rows -- and who takes them"""
    import test_gpu_fir_runs as T
    from dspeed_amd.chain import plan
    from dspeed_amd.errors import DSPFatal

    k12 = K.taps_of(K.V(4, 1, 7), "exact")

    def planned(n, taps, mode="s", offset=0, stride=None, **kw):
        return plan(T._program(n, offset, n + offset if stride is None else stride, taps, mode, **kw)[0])

    assert planned(64, k12)["kernel"] == "dsp_fir_runs_kernel" and K.admitted(64, 12, "s")
    refused = [(dict(n=60), dict()), (dict(n=20), dict()), (dict(n=64, offset=2, stride=72), dict(offset=2, stride=72)), (dict(n=64, stride=66), dict(stride=66)),
               (dict(n=64, dtype=np.int16), dict(dtype=np.int16))]
    for kw, adm in refused:
        for reductions in (True, False):
            p = planned(taps=k12, reductions=reductions, **kw)
            assert p["kernel"] == "dsp_vm_kernel<float>", (kw, p["kernel"])
            assert not reductions or "float32, 16-byte aligned and a multiple of 8 samples" in p["note"]
        assert not K.admitted(kw["n"], 12, "s", **adm)
    # 513 taps: the interpreter where values are read off the filtered waveform, the matrix-core FIR where it is only kept
    k513 = K.taps_of(K.V(13, 500), "exact")
    assert planned(1024, k513)["kernel"] == "dsp_vm_kernel<float>" and planned(1024, k513, reductions=False)["kernel"] == "dsp_fir_f16_kernel"
    assert not K.admitted(1024, 513, "s") and K.admitted(1024, 512, "s")
    assert planned(1024, K.taps_of(K.V(12, 500), "exact"))["kernel"] == "dsp_fir_runs_kernel"
    # a kernel longer than the row: nobody's (convolutions.py raises as well)
    for mode in "sf":
        with pytest.raises(DSPFatal, match="longer than the input"):
            planned(8, K.taps_of(K.V(4, 5), "exact"), mode)
        assert not K.admitted(8, 9, mode)
    assert planned(8, K.taps_of(K.V(3, 5), "exact"), "v")["kernel"] == "dsp_fir_runs_kernel"
    # without the hint the kernel is never chosen
    assert planned(64, k12, hint=0)["kernel"] == "dsp_vm_kernel<float>"


def test_the_compiler_and_the_prep_kernel_agree_on_what_is_piecewise_constant():
    from dspeed_amd import compiler

    rng = np.random.default_rng(15)
    seen = {"taken": 0, "many": 0, "nonfinite": 0, "25": 0, "26": 0, "negzero": 0}
    for i in range(3000):
        n_runs = int(rng.integers(1, 40))
        vals = rng.choice(np.float32([-2, -1, -0.0, 0.0, 0.5, 1, 3]), n_runs)
        k = np.repeat(vals, rng.integers(1, 1 + 512 // n_runs, n_runs)).astype(np.float32)[:K.MAX_TAPS]
        if i % 9 == 0:
            k[int(rng.integers(len(k)))] = rng.choice(np.float32([np.nan, np.inf, -np.inf]))
        t, w, raw, finite = K.breakpoints(k)
        took = compiler._piecewise_constant(k)
        assert took == (finite and raw <= K.RUNS_MAX + 1), (i, raw, finite)
        # the hint set, the kernel's own look at the taps agrees but for the all-zero kernel, which it does tap by tap
        assert (K.table(k) is not None) == (took and raw > 0)
        seen["taken" if took else ("nonfinite" if not finite else "many")] += 1
        seen["25"] += finite and raw == 25
        seen["26"] += finite and raw == 26
        seen["negzero"] += bool(((k[1:] == 0) & (k[:-1] == 0) & (np.signbit(k[1:]) != np.signbit(k[:-1]))).any())
    assert min(seen.values()) >= 10, seen
    assert not compiler._piecewise_constant(np.zeros(513, np.float32)) and compiler._piecewise_constant(np.zeros(16, np.float32))
    for c in CASES:
        if not c.tap_nan:
            assert compiler._piecewise_constant(K.taps(c, "exact")) == (K.breakpoints(K.taps(c, "exact"))[2] <= 25)


def test_the_recipe_cases_compile_onto_the_kernel():
    from dspeed_amd.processing_chain import WaveformInput, build_processing_chain

    for c in CASES:
        if not c.recipe:
            continue
        for keep in (True, False):
            recipe, names = K.recipe(c, "exact", keep)
            x = K.rows_of(c.id, "exact")
            tb = {"waveform": WaveformInput(np.array(x), 1.0, 0.0), "thr": K.thresholds(c.id, "exact", len(x))}
            chain, _, out = build_processing_chain(recipe, tb)
            assert [out[k].shape for k in names] == [(len(x),)] * 5 + ([(len(x), c.P)] if keep else [])
