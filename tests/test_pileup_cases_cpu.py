"""The case book of the pile-up finder (tests/pileup_cases.py) against the reference bodies' recorded results (tests/golden/pileup.npz,
tools/gen_golden_pileup.py): the emulation -- the yardstick of the GPU tests -- equals what rc_cr2 and bi_level_zero_crossing_time_points
returned under CPython bit for bit with CPython's cube, and differs from it with numba's where, and only where, pow(a, 3) and
a * (a * a) differ; the reference's own counting of the sample-0 row and its twin."""
import json
import math
import os

import numpy as np
import pytest

import pileup_cases as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"{pc.BOOK}.npz")


@pytest.fixture(scope="module")
def book():
    return np.load(GOLDEN)


def _pole(book, loop, tau):
    """the pole the reference run computed (recorded: the last bit of exp is the library's)"""
    return pc.NAN if tau != tau else float(book[f"pole_{loop}_tau{tau}/a"])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def test_the_fixture_holds_data_only_and_every_case(book):
    keys = {e["case"] for e in json.loads(str(book["__index__"]))}
    for loop in pc.LOOPS:
        assert {k for k, _n, _t in pc.filter_cases(loop)} <= keys and {c["key"] for c in pc.walk_cases(loop)} <= keys
        assert {pc.fused_case(loop, *f)["key"] for f in pc.FUSED} <= keys
    assert os.path.getsize(GOLDEN) < 600 * 1024
    assert all(v.dtype.kind in "fu" or k == "__index__" for k, v in book.items())
    assert max(v.shape[-1] for k, v in book.items() if k != "__index__" and v.ndim) <= 257


def test_the_recorded_poles_are_this_machines_to_the_last_bit_or_the_one_before(book):
    for loop, T in pc.LOOPS.items():
        for tau in pc.TAUS:
            a = _pole(book, loop, tau)
            for exp in ("numpy", "libm"):
                assert abs(pc.pole(tau, T, exp) - a) <= np.spacing(a), (loop, tau, exp)
    assert pc.pole(20, np.float32, "libm") == math.exp(-1 / 20) and np.isnan(pc.pole(pc.NAN, np.float32))


@pytest.mark.parametrize("loop", ["f32", "f64"])
def test_rc_cr2_with_cpythons_cube_equals_the_reference_bit_for_bit(book, loop):
    T = pc.LOOPS[loop]
    fatal_rows = [pc.FILTER_FAMILIES.index(f) for f in pc.FILTER_FATAL]
    for key, n, tau in pc.filter_cases(loop):
        out, fatal = pc.emulate_rc_cr2(pc.filter_rows(loop, n), tau, T, cube="pow", a=_pole(book, loop, tau))
        assert _same(out, book[f"{key}/out"]), key
        assert np.array_equal(fatal, book[f"{key}/fatal"] != 0), key
        # which rows raise: an infinite first sample wherever the recursion reads it twice (n >= 6); never a NaN row, never a NaN t_tau
        assert list(np.flatnonzero(fatal)) == (fatal_rows if n >= 6 and tau == tau else []), key
        for f in ("nan-first", "nan-middle", "nan-last"):
            assert np.isnan(out[pc.FILTER_FAMILIES.index(f)]).all(), (key, f)
        if tau != tau:
            assert np.isnan(out).all(), key
        assert _same(out[:, :3][~np.isnan(out[:, 0])], pc.filter_rows(loop, n)[:, :3][~np.isnan(out[:, 0])]), key


def test_numbas_cube_differs_where_pow_does_and_nowhere_else(book):
    """float64 loop: at tau 20 and 100 pow(a, 3) != a * (a * a) and rows change bits; at tau 500 they are equal and no row does"""
    for tau, differs in ((20, True), (100, True), (500, False)):
        a = np.float64(_pole(book, "f64", tau))
        assert (a**3 != a * (a * a)) == differs and a**2 == a * a, tau
        changed = 0
        for key, n, t in pc.filter_cases("f64"):
            if t == tau:
                out, _ = pc.emulate_rc_cr2(pc.filter_rows("f64", n), tau, np.float64, cube="product", a=a)
                want = book[f"{key}/out"]
                changed += int((~np.isnan(want) & (out != want)).sum())
        assert (changed > 0) == differs, (tau, changed)
        print(f"tau {tau}: {changed} samples of the float64 book change bits under the product rule")


@pytest.mark.parametrize("loop", ["f32", "f64"])
def test_the_walk_equals_the_reference_bit_for_bit(book, loop):
    T = pc.LOOPS[loop]
    over = 0
    for c in pc.walk_cases(loop):
        count, polarity, times = pc.emulate_walk(c["rows"], c["pos"], c["neg"], c["gate"], c["t_start"], c["m"], T)
        key = c["key"]
        assert np.array_equal(count, book[f"{key}/count"]) and count.dtype == np.uint32, key
        assert _same(polarity, book[f"{key}/polarity"]) and _same(times, book[f"{key}/times"]), key
        over += int((count > c["m"]).sum())
        row = dict(zip(c["names"], count))
        # the gate is strict: i - state is 4 on this row; int() cuts a fractional gate towards zero
        assert row["gate4"] == row["gate4.5"] == row["gate4.999"] == row["gate0"] == row["gate-1"] == row["gate-0.5"] == 0, key
        if c["n"] >= 16:
            assert row["gate5"] == row["gate5.5"] == row["gate8"] == row["gate3000000000.0"] > 0, key
            assert row["alternating-overflow"] >= (c["n"] - 2) // 2, key  # a crossing every other sample
        for name in ("nan", "nan-pos", "nan-neg", "nan-start", "nan-start-nan-row", "mono-up", "mono-down", "zeros", f"start{c['n'] - 1}"):
            assert row[name] == 0, (key, name)
            if name.startswith("nan"):
                assert np.isnan(polarity[c["names"].index(name)]).all() and np.isnan(times[c["names"].index(name)]).all()
    assert over > 50  # the count goes on past the lists' length


@pytest.mark.parametrize("loop", ["f32", "f64"])
def test_the_walk_of_filtered_rows_equals_the_reference(book, loop):
    T = pc.LOOPS[loop]
    found = 0
    for f in pc.FUSED:
        c = pc.fused_case(loop, *f)
        filtered, fatal = pc.emulate_rc_cr2(c["rows"], c["tau"], T, cube="pow", a=_pole(book, loop, c["tau"]))
        assert not fatal.any()
        count, polarity, times = pc.emulate_walk(filtered, c["pos"], c["neg"], c["gate"], c["t_start"], c["m"], T)
        assert np.array_equal(count, book[f"{c['key']}/count"]) and _same(polarity, book[f"{c['key']}/polarity"]) and _same(times, book[f"{c['key']}/times"])
        found += int(count.sum())
    assert found > 20


def test_a_threshold_crossing_at_sample_0_counts_as_not_set(book):
    """the two rows the issue quotes, as the reference counted them, and as the emulation does"""
    for name, row, n, t, p in (("sample0", pc.SAMPLE0, 2, [2, 4], 0), ("sample0_twin", pc.SAMPLE0_TWIN, 3, [2, 4, 6], 1)):
        for count, polarity, times in ((book[f"{name}/count"], book[f"{name}/polarity"], book[f"{name}/times"]),
                                       pc.emulate_walk(np.array([row], np.float64), 1, -1, 10, 0, 5, np.float64)):
            assert count[0] == n and list(times[0, :n]) == t and list(polarity[0, :n]) == [p] * n and np.isnan(times[0, n:]).all()


def test_the_rounding_case_tells_the_stored_row_from_the_state():
    rows, tau, pos, neg, gate, k = pc.rounding_case()
    stored, _ = pc.emulate_rc_cr2(rows, tau, np.float32, exp="libm")
    state, _ = pc.emulate_rc_cr2(rows, tau, np.float32, exp="libm", state=True)
    assert state.dtype == np.float64 and stored[0, k] == pos and state[0, k] > float(pos) and np.float32(state[0, k]) == pos
    of_stored = pc.emulate_walk(stored, pos, neg, gate, 0, 5, np.float32)
    of_state = pc.emulate_walk(state, pos, neg, gate, 0, 5, np.float64)
    assert not np.array_equal(of_stored[0], of_state[0])  # the counts differ: a walk of the state proves nothing about the device
