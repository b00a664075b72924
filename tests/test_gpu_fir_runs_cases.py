"""The run-length FIR kernel at every step, window and group edge (tests/fir_runs_cases.py): every group size at the front, the end and
the middle of a kernel, ramps of 9, 16 and 17 breakpoints, tables of 2 .. 26 entries, windows of 1 .. 512 taps with the last breakpoint at
m, rows of 8 .. 3080 samples in every mode, every cut and vector-store step, kept outputs off 16-byte boundaries, 1 .. 5 rows and more rows
than a round holds, plateaus of equal extremes across lanes and steps, NaNs and infinities.

Every case runs the raw program (LOAD, CONVOLVE with the hint, [STORE], MIN_MAX, AMAX, two walks, two pick-offs) twice, the filtered
waveform kept and not kept, on two families of rows and taps:

  exact     integer run values and rows, every output an integer below 2^24: the int64 convolution, ``np.array_equal``; the per-event
            values are the oracle's on that expectation, not on what the device stored;
  pedestal  rows 1000 + uniform(-1, 1) under run values in +-[0.5, 1] (sum-path cases): the float64 convolution at TOL of the row's
            filtered peak, the per-event values the oracle's on the stored row, bit for bit.

A kept output's buffer starts as a sentinel: nothing outside the rows' P elements may change.  Rows with a NaN or an infinity follow
``oracle.convolve_wf``.  profiles/r15_fir_runs_cases.md holds what the module measured on an MI355X."""
import numpy as np
import pytest

import fir_runs_cases as K
from test_gpu_fir_runs import TOL, _execute, _program, _reductions_of

pytestmark = pytest.mark.gpu
CASES = K.cases()
KERNEL = "dsp_fir_runs_kernel"
WORST = {}  # class -> the largest pedestal deviation over the bar's scale


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    for name in sorted(WORST):
        print(f"FIGURE class {name}: pedestal worst {WORST[name]:.3e} of the peak")


def _run(c, x, k, thr, keep, walk_from, picks, geometry=None):
    prog, P, outs = _program(c.n, 0, c.n, k, c.mode, keep=keep, walk_from=walk_from, picks=picks, out_offset=c.off, out_stride=c.stride)
    assert P == c.P
    try:
        kernel, got = _execute(prog, outs, P, x, k, thr, 1, keep, out_offset=c.off, out_stride=c.stride, fill=K.SENTINEL, geometry=geometry)
    except RuntimeError as e:  # (the runtime's own error: nothing more is started on a device that may have faulted)
        pytest.exit(f"{c.id}: {e}", returncode=3)
    return kernel, outs, got


def _same(a, b):
    """bit for bit but for the sign of a zero, a NaN equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def hold(c, family, x, k, thr, want_all, found, geometry=None):
    """both runs of one family: the kept output, its buffer and the per-event values, kept and from the scratch row"""
    want, fin, conv, y = want_all
    walk_from, picks = K.walks_and_picks(c)
    kernel, outs, got = _run(c, x, k, thr, True, walk_from, picks, geometry)
    kernel2, outs2, got2 = _run(c, x, k, thr, False, walk_from, picks)
    what = f"{c.id} {family}"
    if KERNEL not in kernel or KERNEL not in kernel2 or outs != outs2:
        found.append(f"{what}: ran on {kernel} / {kernel2}")
        return
    f = got["filtered"]
    outside = np.ones(got["filtered_buffer"].shape, dtype=bool)
    outside[:, c.off:c.off + c.P] = False
    if not (got["filtered_buffer"][outside] == K.SENTINEL).all():
        r, col = np.argwhere(outside & (got["filtered_buffer"] != K.SENTINEL))[0]
        found.append(f"{what}: a store outside the row, buffer row {r} element {col}")
    if family == "exact":
        dev = np.abs(f[fin].astype(np.float64) - want[fin])
        print(f"FIGURE {what}: {int(fin.sum())} finite rows, largest |device - int64| {dev.max() if dev.size else 0.0:.6g}")
        if f.dtype != np.float32 or not np.array_equal(f[fin].astype(np.float64), want[fin].astype(np.float64)):
            rows = np.flatnonzero(fin)[np.unique(np.nonzero(dev)[0])][:8].tolist()
            cols = np.unique(np.nonzero(dev)[1])[:12].tolist()
            found.append(f"{what}: not equal to the int64 convolution in rows {rows}, columns {cols}, largest difference {dev.max():g}")
        if not _same(f[~fin], y[~fin]):
            found.append(f"{what}: rows with a NaN / an infinity differ from the oracle's in rows {np.flatnonzero(~fin)[[not _same(a, b) for a, b in zip(f[~fin], y[~fin])]][:8].tolist()}")
        ref = _reductions_of(y, thr, walk_from, picks)  # on the EXPECTED rows
    else:
        peak = np.abs(want).max(axis=1, keepdims=True)
        err = (np.abs(f.astype(np.float64) - want) / peak).max()
        print(f"FIGURE {what}: largest |device - float64| / peak {err:.3e}")
        for name in set(K.classes(c)) & set(K.CLASSES):
            WORST[name] = max(WORST.get(name, 0.0), float(err))
        if not err <= TOL:
            found.append(f"{what}: {err:.3e} of the filtered peak from the float64 convolution")
        ref = _reductions_of(f, thr, walk_from, picks)  # the comparisons and selections on the float32 samples the kernel stored
    for name in outs:
        for label, g in (("kept", got[name]), ("scratch row", got2[name])):
            if not _same(g, ref[name]):
                bad = np.flatnonzero(~((g == ref[name]) | (np.isnan(g) & np.isnan(ref[name]))))
                found.append(f"{what} {label}: {name} differs in rows {bad[:8].tolist()}: {g[bad[:4]].tolist()} for {ref[name][bad[:4]].tolist()}")


@pytest.mark.parametrize("case_id", [c.id for c in CASES if c.pattern != "rounds"])
def test_fir_runs_case(case_id):
    c = K.by_id(case_id)
    found = []
    for family in c.families:
        x, k = K.rows_of(case_id, family), K.taps(c, family)
        geometry = {}
        hold(c, family, x, k, K.thresholds(case_id, family, len(x)), K.expect(case_id, family), found, geometry)
        assert geometry["waves_per_block"] == 4 and geometry["lds_bytes_per_wave"] == K.lds_bytes(c.m) // 4 and geometry["blocks"] == (len(x) + 3) // 4
    for f in found:
        print("DIFFERS", f)
    assert not found, found[:8]


def test_more_rows_than_a_round_holds():
    """Every wavefront of the launch takes a second row: the window re-zeroed, the carry reset, the scratch row used again.  The rows of
    the first round hold integers up to +-200 (a NaN row, a row with +inf and one with -inf in every sixteen), the rows that follow them on
    the same wavefronts integers in [-1, 1]: what a wavefront kept from its first row would be many times its second row's output.  The
    number of rows comes from the chain's own launch geometry"""
    from dspeed_amd.chain import Chain

    c = next(c for c in CASES if c.pattern == "rounds")
    walk_from, picks = K.walks_and_picks(c)
    prog, _, _ = _program(c.n, 0, c.n, K.taps(c, "exact"), c.mode, keep=False, walk_from=walk_from, picks=picks)
    ch = Chain(prog, "fir runs geometry", np.float32)
    assert ch.set_fused(1)
    lo, hi = 1, 1 << 22  # the fewest rows whose launch has fewer wavefronts than rows
    assert 4 * ch.geometry(hi)["blocks"] < hi
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if 4 * ch.geometry(mid)["blocks"] < mid else (mid + 1, hi)
    n_rows = lo + 3
    n_waves = 4 * ch.geometry(n_rows)["blocks"]
    assert n_waves < n_rows <= 2 * n_waves and n_rows * c.n * 4 <= 8 << 20, (n_rows, n_waves)
    print(f"FIGURE {c.id}: {n_rows} rows on {n_waves} wavefronts")
    found = []
    for family in c.families:
        x, k = K.rows_of(c.id, family, n_rows, n_waves), K.taps(c, family)
        want_all = K.expect(c.id, family, n_rows, n_waves)
        if family == "exact":  # a finite row of small integers behind a NaN row, behind an infinity row and behind a row of large ones
            fin = want_all[1]
            follows = np.arange(n_waves, n_rows) - n_waves
            assert fin[n_waves:].all() and (~fin[follows]).sum() >= 100 and np.isnan(x[follows]).any() and np.isposinf(x[follows]).any()
            assert np.abs(want_all[0][:n_waves]).max() > 50 * np.abs(want_all[0][n_waves:]).max() > 0
        geometry = {}
        hold(c, family, x, k, K.thresholds(c.id, family, n_rows), want_all, found, geometry)
        assert 4 * geometry["blocks"] == n_waves
    for f in found:
        print("DIFFERS", f)
    assert not found, found[:8]


@pytest.mark.parametrize("case_id", [c.id for c in CASES if c.recipe])
def test_recipe_equals_the_raw_program(case_id):
    """convolve_wf (taps from loadlh5) -> min_max -> time_point_thresh through build_processing_chain, the filtered waveform an output or
    not: on dsp_fir_runs_kernel unless the kernel has 26 breakpoints, and bit for bit what the raw program gives -- which is the int64
    convolution and the oracle's values on it"""
    from dspeed_amd.processing_chain import WaveformInput, build_processing_chain

    c = K.by_id(case_id)
    x, k = K.rows_of(case_id, "exact"), K.taps(c, "exact")
    thr = K.thresholds(case_id, "exact", len(x))
    want, fin, conv, y = K.expect(case_id, "exact")
    assert fin.all()
    prog, P, outs = _program(c.n, 0, c.n, k, c.mode, keep=True, walk_from=("t_max",), picks=())
    try:
        kernel, raw = _execute(prog, outs, P, x, k, thr, 1, True)
    except RuntimeError as e:
        pytest.exit(f"{case_id}: {e}", returncode=3)
    assert KERNEL in kernel
    assert np.array_equal(raw["filtered"].astype(np.float64), want.astype(np.float64))
    ref = _reductions_of(y, thr, ("t_max",), ())
    for keep in (True, False):
        recipe, names = K.recipe(c, "exact", keep)
        try:
            chain, _, out = build_processing_chain(recipe, {"waveform": WaveformInput(np.array(x), 1.0, 0.0), "thr": thr})
            chain.execute()
        except RuntimeError as e:
            pytest.exit(f"{case_id} recipe: {e}", returncode=3)
        on_runs = any(KERNEL in name for _what, name in chain.kernels())
        assert on_runs == c.sum_path, (keep, chain.kernels())
        for name in ("t_min", "t_max", "a_min", "a_max", "walk0"):
            assert _same(np.asarray(out[name]), raw[name]) and _same(raw[name], ref[name]), (keep, name, out[name], raw[name], ref[name])
        if keep:
            assert _same(np.asarray(out["wf_f"]), raw["filtered"])
