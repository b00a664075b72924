"""The case book of the decay-tail fitter (tests/tailfit_cases.py) against the reference bodies' recorded results (tests/golden/tailfit.npz,
tools/gen_golden_tailfit.py, the bodies run with numba's typing): the emulation -- the yardstick of the GPU tests -- equals poly_diff and
log_check's NaN pattern bit for bit in both loops; poly_fit, whose matrix product is the BLAS's there, is held to the derived bound of its
sums; poly_exp_rms and log_check's values to the running error bound of the case module, which takes the one-ulp accuracy of the
exponentials and logarithms involved.  The worst ratio to each bound is printed."""
import json
import os

import numpy as np
import pytest

import tailfit_cases as tc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"{tc.BOOK}.npz")


@pytest.fixture(scope="module")
def book():
    return np.load(GOLDEN)


def test_the_fixture_holds_data_only_and_every_case(book):
    keys = {e["case"] for e in json.loads(str(book["__index__"]))}
    for loop in tc.LOOPS:
        assert {f"log_{loop}_n{n}" for n in tc.LENGTHS} <= keys
        assert {f"{k}_{loop}_n{n}_m{m}" for n, m in tc.fit_cases() for k in ("fit", "fitlog")} <= keys
        assert {f"{k}_{loop}_n{n}_m{m}" for n in tc.LENGTHS for m in tc.MS for k in ("diff", "exp")} <= keys
    assert os.path.getsize(GOLDEN) < 600 * 1024
    assert all(v.dtype.kind == "f" or k == "__index__" for k, v in book.items())
    assert max(v.shape[-1] for k, v in book.items() if k != "__index__" and v.ndim) <= max(max(tc.LENGTHS), len(tc.FAMILIES) * len(tc.PAR_FAMILIES))


def test_the_book_covers_what_the_issue_names():
    assert tc.LENGTHS == (1, 2, 3, 63, 64, 65, 129) and tc.ROW_COUNTS == (1, 63, 64, 65, 130) and tc.MS == (1, 2, 4, 8) and tc.POLY_MAX == 8
    rows = tc.tail_rows("f64", 65)
    f = tc.FAMILIES.index
    assert (rows[f("decay")] > 0).all() and (np.diff(rows[f("decay")]) != 0).all() and rows[f("zero"), 32] == 0 and rows[f("negative"), 64] < 0
    assert np.isnan(rows[f("nan-first"), 0]) and np.isnan(rows[f("nan-middle"), 32]) and np.isnan(rows[f("nan-last"), 64]) and np.isposinf(rows[f("inf"), 21])
    pars = tc.coefficients("f64", 4, 65)
    assert np.isnan(pars[tc.PAR_FAMILIES.index("nan")]).any() and not np.isnan(np.delete(pars, tc.PAR_FAMILIES.index("nan"), axis=0)).any()
    # the overflow: exp(temp) leaves float64 inside the row, and the sums with it
    mean, rms = tc.emulate_residual(rows[[f("decay")]], pars[[tc.PAR_FAMILIES.index("overflow")]], np.float64, True)
    assert np.isneginf(mean[0]) and np.isposinf(rms[0])
    assert all(np.linalg.matrix_rank(tc.inverse(n, m - 1)) == m for n, m in tc.fit_cases() if m <= 2)
    with pytest.raises(np.linalg.LinAlgError):
        tc.inverse(2, 3)


@pytest.mark.parametrize("loop", ["f32", "f64"])
def test_log_check_the_nan_pattern_exactly_the_values_within_the_bound(book, loop):
    T, worst = tc.LOOPS[loop], 0.0
    for n in tc.LENGTHS:
        rows, ref = tc.tail_rows(loop, n), book[f"log_{loop}_n{n}/out"]
        mine = tc.emulate_log_check(rows, T)
        assert mine.dtype == ref.dtype == np.dtype(T) and np.array_equal(np.isnan(mine), np.isnan(ref)), n
        bad = [tc.FAMILIES.index(name) for name in tc.BAD_FOR_LOG]
        assert np.isnan(ref[bad]).all() and not np.isnan(np.delete(ref, bad, axis=0)).any(), n
        exact, bound = tc.log_bound(rows, T)
        for got in (mine, ref):
            ok, ratio = tc.within(got, exact, bound, mine)
            assert ok, (n, ratio)
            worst = max(worst, ratio)
    print(f"log_check {loop}: worst |got - exact| / bound = {worst:.3g}")


@pytest.mark.parametrize("loop", ["f32", "f64"])
def test_poly_fit_within_the_bound_of_its_sums(book, loop):
    T, worst = tc.LOOPS[loop], 0.0
    for n, m in tc.fit_cases():
        inv = book[f"fit_{loop}_n{n}_m{m}/inv"]
        assert inv.shape == (m, m) and inv.dtype == np.float64
        for name, rows in (("fit", tc.tail_rows(loop, n)), ("fitlog", tc.emulate_log_check(tc.tail_rows(loop, n), T))):
            ref = book[f"{name}_{loop}_n{n}_m{m}/pars"]
            mine = tc.emulate_poly_fit(rows, inv, T)
            assert mine.dtype == ref.dtype == np.dtype(T) and mine.shape == ref.shape == (len(rows), m)
            nan_rows = np.isnan(rows).any(axis=1)
            assert np.isnan(mine[nan_rows]).all() and np.isnan(ref[nan_rows]).all(), (name, n, m)  # (the reference: untouched, NaN as handed in)
            exact, bound = tc.fit_bound(rows, inv, T)
            for got in (mine, ref):
                ok, ratio = tc.within(got, exact, bound, mine)
                assert ok, (name, n, m, ratio)
                worst = max(worst, ratio)
    print(f"poly_fit {loop}: worst |got - exact| / bound = {worst:.3g}")


def test_the_inverse_is_the_factorys_and_this_machines_to_rounding(book):
    from dspeed_amd.processors import poly_fit_inverse

    for n, m in tc.fit_cases():
        mine, ref = tc.inverse(n, m - 1), book[f"fit_f64_n{n}_m{m}/inv"]
        assert np.array_equal(poly_fit_inverse(n, m - 1), mine) and np.array_equal(ref, book[f"fit_f32_n{n}_m{m}/inv"])
        if m <= 2:  # (well conditioned: the LAPACK of this machine agrees with the recorded one to a few units)
            assert np.allclose(mine, ref, rtol=1e-12, atol=0), (n, m)


@pytest.mark.parametrize("loop", ["f32", "f64"])
def test_poly_diff_equals_the_reference_bit_for_bit(book, loop):
    T = tc.LOOPS[loop]
    for n in tc.LENGTHS:
        for m in tc.MS:
            rows, pars = tc.residual_case(loop, n, m)
            mean, rms = tc.emulate_residual(rows, pars, T, False)
            assert tc.same(mean, book[f"diff_{loop}_n{n}_m{m}/mean"]) and tc.same(rms, book[f"diff_{loop}_n{n}_m{m}/rms"]), (n, m)
            bad = np.isnan(rows).any(axis=1) | np.isnan(pars).any(axis=1)
            assert np.isnan(mean[bad]).all() and np.isnan(rms[bad]).all() and not np.isnan(mean[~bad & np.isfinite(rows).all(axis=1)]).any()
            if n == 1:  # rms /= 0: no error, the IEEE result
                assert not np.isfinite(rms).any()


@pytest.mark.parametrize("loop", ["f32", "f64"])
def test_poly_exp_rms_within_the_running_error_bound(book, loop):
    T, worst = tc.LOOPS[loop], [0.0, 0.0]
    for n in tc.LENGTHS:
        for m in tc.MS:
            rows, pars = tc.residual_case(loop, n, m)
            mean, rms = tc.emulate_residual(rows, pars, T, True)
            x_mean, x_rms, b_mean, b_rms = tc.residual_bound(rows, pars, T, True)
            for k, (mine, ref, exact, bound) in enumerate(((mean, book[f"exp_{loop}_n{n}_m{m}/mean"], x_mean, b_mean), (rms, book[f"exp_{loop}_n{n}_m{m}/rms"], x_rms, b_rms))):
                for got in (mine, ref):
                    ok, ratio = tc.within(got, exact, bound, mine)
                    assert ok, (n, m, "mean rms".split()[k], ratio)
                    worst[k] = max(worst[k], ratio)
    print(f"poly_exp_rms {loop}: worst |got - exact| / bound = {worst[0]:.3g} (mean), {worst[1]:.3g} (rms)")


@pytest.mark.parametrize("loop", ["f32", "f64"])
def test_the_bound_also_holds_poly_diff(loop):
    """the same running bound with the polynomial in the exponential's place: the exact test above is the stronger one; this one checks the bound"""
    T = tc.LOOPS[loop]
    for n, m in ((65, 4), (129, 8), (3, 2)):
        rows, pars = tc.residual_case(loop, n, m)
        mean, rms = tc.emulate_residual(rows, pars, T, False)
        x_mean, x_rms, b_mean, b_rms = tc.residual_bound(rows, pars, T, False)
        assert tc.within(mean, x_mean, b_mean, mean)[0] and tc.within(rms, x_rms, b_rms, rms)[0], (n, m)
