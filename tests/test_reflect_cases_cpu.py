"""The case book of reflected_convolve_wf (tests/reflect_cases.py) against the reference body's recorded results
(tests/golden/reflected_convolve.npz, tools/gen_golden_reflect.py): ``emulate`` -- the yardstick of the GPU tests -- is held to what
np.convolve over np.pad(mode="reflect") gave, exactly on the integer class and within the project's FIR bars elsewhere; five wrong
neighbours of the rule each fail on the book; the host generator gaussian_filter1d against its fixture values."""
import json
import os

import numpy as np
import pytest

import reflect_cases as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"{rc.BOOK}.npz")


@pytest.fixture(scope="module")
def book():
    return np.load(GOLDEN)


def _kernel(book, key, name, k):
    """the taps the reference ran with: the book's, but for the Gaussian ones, which the reference's own generator made (recorded)"""
    return book[f"{key}/kernel"] if name == "gauss" else k


def test_the_fixture_holds_data_only_and_every_case_of_its_part(book):
    index = json.loads(str(book["__index__"]))
    keys = {e["case"] for e in index}
    for loop in ("f32", "f64"):
        for key, n, m, name, _k in rc.fixture_cases(loop):
            assert key in keys and book[f"{key}/{loop}"].shape == (len(rc.families(loop)), n)
    assert os.path.getsize(GOLDEN) < 600 * 1024
    assert all(v.dtype.kind == "f" or k == "__index__" for k, v in book.items())


def test_the_integer_class_equals_the_reference_float32_output_exactly(book):
    """integer rows |x| <= 2^11 under integer taps |k| <= 2^4, m <= 2^8: every partial sum below 2^23, so float32 summation is exact in any
    order and np.convolve's float32 result is what any correct evaluation gives"""
    checked = 0
    for key, n, m, name, k in rc.fixture_cases("f32"):
        if not rc.integer_class("f32", n, m, name):
            continue
        fin = rc.finite_rows("f32")
        got = rc.emulate(rc.rows_of("f32", n), k, np.float32)
        assert np.array_equal(got[fin], book[f"{key}/f32"][fin]), key
        assert np.abs(got[fin]).max() < 2 ** 23 and np.abs(rc.rows_of("f32", n)[fin]).max() <= 2 ** 11 and np.abs(k).max() <= 2 ** 4
        checked += 1
    assert checked > 50
    for key, n, m, name, k in rc.fixture_cases("f64"):
        if rc.integer_class("f64", n, m, name):
            fin = rc.finite_rows("f64")
            assert np.array_equal(rc.emulate(rc.rows_of("f64", n), k, np.float64)[fin], book[f"{key}/f64"][fin]), key


@pytest.mark.parametrize("loop, ref, bar", [("f32", "f64_of_f32", 1e-6), ("f64", "f64", 1e-12)])
def test_every_finite_case_within_the_fir_bar_of_the_float64_body(book, loop, ref, bar):
    """1e-6 x max|reference row| in the float32 loop, 1e-12 in the float64 loop: the project's FIR bars"""
    worst = 0.0
    for key, n, m, name, k in rc.fixture_cases(loop):
        if name == "nan":
            continue
        want = book[f"{key}/{ref}"]
        got = rc.emulate(rc.rows_of(loop, n), _kernel(book, key, name, k), rc.LOOPS[loop])
        for r in rc.finite_rows(loop):
            peak = np.abs(want[r]).max()
            if peak == 0:
                assert not got[r].any(), key
                continue
            err = np.abs(got[r].astype(np.float64) - want[r]).max() / peak
            worst = max(worst, err)
            assert err <= bar, (key, r, err)
    print(f"{loop}: worst distance from the float64 body {worst:.3g} of the row's peak (bar {bar:g})")


@pytest.mark.parametrize("loop", ["f32", "f64"])
def test_non_finite_cases_have_the_reference_s_pattern(book, loop):
    seen = set()
    for key, n, m, name, k in rc.fixture_cases(loop):
        want = book[f"{key}/{loop}"]
        got = rc.emulate(rc.rows_of(loop, n), _kernel(book, key, name, k), rc.LOOPS[loop])
        for what, test in (("nan", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
            assert np.array_equal(test(got), test(want)), (key, what)
            if test(want).any():
                seen.add(what)
        if name == "nan":
            assert np.isnan(want).all()
        fams = rc.families(loop)
        for f in ("nan-first", "nan-middle", "nan-last"):
            assert np.isnan(want[fams.index(f)]).all(), (key, f)
        if name == "zero" and m >= 2:  # +inf under a zero tap: NaN where the window covers it, and only there
            row = want[fams.index("inf")]
            assert np.isnan(row).any() and (n <= m + 1 or not np.isnan(row).all()), key
    assert seen == {"nan", "+inf", "-inf"}


def test_each_wrong_neighbour_fails_on_the_book():
    """'symmetric' padding, a centre of m // 2, an unflipped kernel, a margin one sample short, and a sample of both margins written to one
    only (m = n): each differs from the rule on at least one case -- and which class of cases catches it"""
    caught = {v: set() for v in rc.WRONG}
    for n, m in [p for p in rc.pairs("f32") if p[0] <= 65]:
        w = rc.rows_of("f32", n)[rc.finite_rows("f32")]
        k = rc.asymmetric(m)
        right = rc.emulate(w, k, np.float32)
        for v in rc.WRONG:
            if not np.array_equal(rc.emulate(w, k, np.float32, variant=v), right):
                caught[v].add("m = 1" if m == 1 else "m = n" if m == n else "even m" if m % 2 == 0 else "odd m")
    assert all(caught.values()), caught
    assert "m = 1" not in caught["symmetric"] | caught["unflipped"] | caught["short-margin"]  # (one tap reaches no margin and has no order)
    assert caught["symmetric"] >= {"even m", "odd m", "m = n"}  # every kernel that reaches a margin
    assert "even m" in caught["centre"]  # (m - 1) // 2 == m // 2 for odd m: only even kernels tell
    assert "odd m" not in caught["centre"] and "m = 1" not in caught["centre"]
    assert caught["unflipped"] >= {"even m", "odd m"}  # the kernels are asymmetric
    assert caught["short-margin"] >= {"even m", "odd m"}
    assert caught["one-edge"] == {"m = n"}  # only there a sample stands in both margins
    print({v: sorted(c) for v, c in caught.items()})


@pytest.mark.parametrize("loop, T, ulps", [("f32", np.float32, 1), ("f64", np.float64, 4)])
def test_gaussian_filter1d_against_its_fixture_values(book, loop, T, ulps):
    """exp evaluated in float64, normalised, rounded once into the array.  NumPy's exp differs between builds in the last bit (DESIGN
    section 2): one float64 ulp of a weight, which the sum and the division may pass on -- at most one ulp after the rounding to float32,
    a few in float64"""
    from dspeed_amd.processors import gaussian_filter1d

    for sigma, truncate in rc.GAUSS:
        want = book[f"gauss_{loop}_s{sigma}_t{truncate}/weights"]
        k = np.empty(len(want), T)
        assert gaussian_filter1d(T(sigma), T(truncate), k) is k
        assert k.dtype == want.dtype and (np.abs(k - want) <= ulps * np.spacing(np.abs(want))).all(), (sigma, truncate)
        assert abs(float(k.astype(np.float64).sum()) - 1) < 1e-6 and np.array_equal(k, k[::-1])


def test_gaussian_filter1d_refusals():
    from dspeed_amd.processors import gaussian_filter1d

    with pytest.raises(ValueError, match="gaussian_filter1d: weights holds 2 \\* int\\(truncate \\* sigma \\+ 0.5\\) \\+ 1 = 9 values \\(8 given\\)"):
        gaussian_filter1d(1.0, 4.0, np.empty(8, np.float32))
    for sigma in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError, match="gaussian_filter1d: sigma must be positive"):
            gaussian_filter1d(sigma, 4.0, np.empty(9, np.float64))
