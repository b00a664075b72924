"""Every waveform op of the interpreter at the row lengths where its LDS layout changes (tests/op_length_cases.py): 1 .. 3073 samples
across one lane's chunk (15 / 16 / 17), the wavefront's 64 chunks (63 / 64 / 65), the growth of the chunk (1023 / 1024 / 1025, 2047 /
2049, 3073) and the route flips of form A (67 / 68 / 69), on 70 rows made so that a pad read as a sample shows -- in float32, float64
and int16.

One test per (op, row type).  It walks the lengths and, for every set of parameters the rules give at that length, runs three forms:

  A  the processor of dspeed_amd.processors (default routing: the reduce, rows and FIR kernels where the planner admits them);
  B  a recipe kept whole on the interpreter, the op reading the loaded rows;
  C  the same with the op reading ``wf_c = waveform + 0`` beside a numpy.amax, an output waveform stored and read by a min_max.

Held, at the bars of test_gpu_processors.py and test_gpu_edges.py and no others: every output against the oracle on the same bits in the
loop's type (bit-exact but for the filters: FILTER_TOL of the row's peak in float32, FILTER_TOL_F64 / DPZ_TOL_F64 in float64, the
dot-product bar for FIR outputs); NaN positions equal; below an op's minimum length the oracle's error, raised; forms B and C bit for
bit the same; in form C the amax of wf_c exact and the min_max equal to the oracle's min_max of the very waveform the STORE wrote.

profiles/r10_op_lengths.md holds what the module measured on an MI355X."""
import numpy as np
import pytest

import op_length_cases as K
import oracle
from test_gpu_processors import DPZ_TOL_F64, FILTER_TOL, FILTER_TOL_F64

pytestmark = pytest.mark.gpu

FIR_TOL = 2e-7  # of sum |k| * max |x| (test_gpu_edges.py::test_fir_edges_same_and_full_modes): the error bound of a float32 dot product
# the float64 loop's dot products: the same number of roundings, 3.3 units of float64's 2^-53 for float32's 2^-24
FIR_TOL_F64 = FIR_TOL * 2.0 ** -29


@pytest.fixture(scope="module")
def P():
    from dspeed_amd import processors

    return processors


def _same(a, b, as_type=None):
    """bit for bit, a NaN equal to any NaN (``as_type``: both in that type first)"""
    a, b = np.asarray(a, dtype=as_type), np.asarray(b, dtype=as_type)
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def _rows(mask):
    return np.flatnonzero(mask.reshape(len(mask), -1).any(axis=1))[:6].tolist()


def _kinds_of(mask):
    return sorted({K.KINDS[r % len(K.KINDS)] for r in np.flatnonzero(mask.reshape(len(mask), -1).any(axis=1))})


def hold(case, got, want, bar, w):
    """one output against the oracle's at its bar -> (what differs, or None; the error over the row's peak for a filter bar, or None)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype and case.op == "slice":
        got = got.astype(want.dtype)  # (a unit-stride slice of int16 rows stays int16, like the reference's view: every value is exact)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shape / type {got.shape} {got.dtype}, expected {want.shape} {want.dtype}", None
    nan = np.isnan(got) != np.isnan(want)
    if nan.any():
        return f"NaN positions differ in rows {_rows(nan)} ({_kinds_of(nan)})", None
    inf = np.isinf(got) != np.isinf(want)
    if inf.any():
        return f"infinities differ in rows {_rows(inf)} ({_kinds_of(inf)})", None
    ok = np.isfinite(want)
    g, r = np.where(ok, got, 0).astype(np.float64), np.where(ok, want, 0).astype(np.float64)
    dev = np.abs(g - r)
    f32 = case.ft == np.float32
    x_max = np.max(np.abs(np.where(np.isfinite(w), w, 0).astype(np.float64)), axis=1).reshape((-1,) + (1,) * (got.ndim - 1))
    worst = None
    if bar == "exact":
        allowed = np.zeros_like(dev)
    elif bar[0] in ("peak", "fir"):
        peak = np.max(np.abs(r).reshape(len(r), -1), axis=1).reshape(x_max.shape)
        tol = FILTER_TOL if f32 else (DPZ_TOL_F64 if bar[1] == "dpz" else FILTER_TOL_F64)
        allowed = tol * peak
        if bar[0] == "fir":
            allowed = np.maximum(allowed, (FIR_TOL if f32 else FIR_TOL_F64) * bar[1] * x_max)
        worst = float(np.max(dev / np.where(peak > 0, peak, 1.0)))
    elif bar[0] == "rtol":
        allowed = bar[1] * np.abs(r)
    elif bar[0] == "atol_in":
        allowed = bar[1] * x_max
    else:  # ("fit", ...): test_linear_slope_fit_golden
        tol = 1e-6 if f32 else 1e-12
        allowed = tol * np.abs(r) + tol * x_max / (case.n if bar[1] == "slope" else 1)
    bad = dev > allowed
    if bad.any():
        return f"{'not bit-exact' if bar == 'exact' else 'off the bar ' + str(bar)} in rows {_rows(bad)} ({_kinds_of(bad)}), worst excess {float(np.max(dev - allowed)):.3e}", worst
    return None, worst


def _raised(err):
    from dspeed_amd.errors import DSPFatal

    return {K.FATAL: DSPFatal, K.ZERODIV: ZeroDivisionError}[err]


def run_recipe(case, form):
    """the op's outputs, and in form C the extras, of the recipe kept whole on the interpreter"""
    from dspeed_amd.processing_chain import build_processing_chain

    recipe, table, names, extra = case.recipe(form)
    with K.switches():
        chain, _, out = build_processing_chain(recipe, table)
        chain.execute()
        assert dict(chain.kernels())["program"].startswith("dsp_vm_kernel")
    return [out[k] for k in names], ({"m": out[extra["m"]], "mm": [out[k] for k in extra["mm"]] if "mm" in extra else None} if form == "C" else None)


def run_case(case, P, found, worst):
    want, err = case.expect()
    w = K.in_loop(case.rows, case.tag)
    forms = {}
    for form in "ABC":
        if form == "A" and case.call is None:
            continue
        what = f"{case.id} form {form}"
        try:
            if form == "A":
                got, extra = case.call(P, case.rows, case.cols), None
            else:
                got, extra = run_recipe(case, form)
        except RuntimeError as e:  # (the runtime's own error: nothing more is started on a device that may have faulted)
            pytest.exit(f"{what}: {e}", returncode=3)
        except (_raised(K.FATAL), ArithmeticError, ValueError, TypeError, NotImplementedError) as e:
            if err is None or not isinstance(e, _raised(err)):
                found.append(f"{what}: raised {type(e).__name__} ({str(e).splitlines()[0][:80]}), expected {err or 'results'}")
            continue
        if err is not None:
            found.append(f"{what}: no error, expected {err}")
            continue
        forms[form] = got
        for (name, _length), g, r, bar in zip(case.outs, got, want, case.bars):
            differs, scaled = hold(case, g, r, bar, w)
            if scaled is not None:
                key = (case.name, case.tag)
                if scaled > worst.get(key, (-1.0,))[0]:
                    worst[key] = (scaled, case.n, form)
            if differs:
                found.append(f"{what} {name}: {differs}")
        if extra is not None:
            with np.errstate(all="ignore"):
                if not _same(extra["m"], np.max(w, axis=1)):
                    found.append(f"{what}: amax of wf_c differs from the rows' maximum")
                if extra["mm"] is not None:
                    stored = np.ascontiguousarray(got[0], dtype=case.ft)
                    ref = oracle.min_max(stored)[:4]
                    for k, g, r in zip(("t_min", "t_max", "a_min", "a_max"), extra["mm"], ref):
                        if not _same(g, r):
                            found.append(f"{what}: min_max of the stored output, {k}, differs in rows {_rows(~((g == r) | (np.isnan(g) & np.isnan(r))))}")
    if "B" in forms and "C" in forms:
        for (name, _length), b, c in zip(case.outs, forms["B"], forms["C"]):
            # (a unit-stride slice of the int16 rows themselves stays int16, of wf_c it is float32: the same values)
            if not _same(b, c, case.ft if case.op == "slice" else None):
                found.append(f"{case.id} {name}: forms B and C differ (the layout changed a result)")


@pytest.mark.parametrize("tag", K.TAGS)
@pytest.mark.parametrize("op", list(K.OPS))
def test_op_at_every_length(op, tag, P):
    found, worst, n_cases = [], {}, 0
    for n in K.LENGTHS:
        for case in K.cases(op, n, tag):
            if case.id in K.OVER_THE_BAR:
                continue  # (test_cases_just_over_their_bar)
            run_case(case, P, found, worst)
            n_cases += 1
    for (name, t), (scaled, n, form) in sorted(worst.items()):
        print(f"WORST {name} {t}: |dev| / peak {scaled:.3e} at {n} samples, form {form}")
    print(f"{op} {tag}: {n_cases} cases at {len(K.LENGTHS)} lengths, {len(found)} findings")
    for f in found:
        print("DIFFERS", f)
    assert not found, (op, tag, len(found), found[:12])


@pytest.mark.xfail(strict=True, reason="device and oracle differ by a little more than the bar; the device is no further from a higher-precision "
                                       "evaluation than the oracle is (op_length_cases.OVER_THE_BAR, profiles/r10_op_lengths.md)")
@pytest.mark.parametrize("case_id", list(K.OVER_THE_BAR))
def test_cases_just_over_their_bar(case_id, P):
    """The bars stay where test_gpu_processors.py has them, and these cases stay visible.  Measured on an MI355X, all three forms alike:

    moving_window_multi, 3 windows of n // 10 samples, float32, all-positive row 22 (3000 +- 50): |device - oracle| is 1.14e-6 of the
    row's peak at 1025 samples (mw_type 1) and 1.06e-6 at 2047 (mw_type 0), the bar 1e-6.  Both run the float32 recurrence w_out[i] =
    w_out[i - 1] + (w[i] - w[i - L]) / L, whose roundings add up like a random walk; against the same recurrence in float64 the worst row
    of those batches is off by 3.05e-6 / 3.02e-6 on the device and 3.05e-6 / 3.17e-6 in the oracle.

    mean_below_threshold, float64, 2047 samples, pulse row 37: the samples below the threshold have a mean magnitude of 131 and a mean of
    -0.0078; device and oracle differ by 2.6e-12 of that mean (the bar: rtol 1e-13, atol 0).  The exact mean (math.fsum) is 2.7e-13 from
    the device's and 2.4e-12 from the oracle's sequential sum."""
    case = next(c for c in K.cases(case_id.split("-")[0], int(case_id.split("-")[-2]), case_id.split("-")[-1]) if c.id == case_id)
    found = []
    run_case(case, P, found, {})
    assert not found, found
