"""The case book of interpolating_upsampler without a device: the emulation of numba's typing (tests/interp_cases.py) against what the
reference's own body wrote (tests/golden/interp_upsampler.npz, tools/gen_golden_interp.py), bit for bit; the NumPy model of the kernel's
formulation -- every output looks its segment up, the spline's second derivatives come from warm-up sweeps over chunks -- against the
emulation, bit for bit, over the whole book; and the wrong neighbours the book catches."""
import json
import os

import numpy as np
import pytest

import interp_cases as ic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", ic.BOOK + ".npz")


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.isnan(a), np.isnan(b))


def test_the_emulation_is_the_references_body_bit_for_bit():
    """CPython ran the body: its powers are C's pow (``powers="libm"``); everything else is the typing the device follows.  On the float32
    loop's integer rows the body ran on a float64 copy and rounded at the store: the emulation runs its float32 typing and agrees."""
    z = np.load(GOLDEN)
    index = json.loads(str(z["__index__"]))
    assert [(e["params"]["n"], e["params"]["m"]) for e in index if e["dtype"] == "f64"] == ic.fixture_pairs()
    seen = set()
    for e in index:
        n, m, loop = e["params"]["n"], e["params"]["m"], e["dtype"]
        assert e["arrays"] == sorted(ic.modes_of(n, m)) and e["kernel"] == ic.KERNEL
        w = ic.fixture_rows(loop, n).astype(ic.LOOPS[loop])
        for mode in e["arrays"]:
            ref = z[f"{e['case']}/{mode}"]
            assert _same(ic.emulate(w, mode, m, powers="libm"), ref), (e["case"], mode)
            if mode in "infcl":  # no powers: numba's variant is the same computation
                assert _same(ic.emulate(w, mode, m), ref), (e["case"], mode)
            seen.add((loop, mode))
    assert seen == {(loop, mode) for loop in ("f32", "f64") for mode in ic.MODES}
    for pair in ic.NAMED_PAIRS + list(ic.FLOAT_BOUND_PAIRS.values()):
        assert pair in ic.fixture_pairs()


def test_the_two_power_rules_differ_in_the_cube_alone():
    """what separates CPython's run of the body from numba's: x * (x * x) against pow(x, 3); x * x is pow(x, 2)"""
    t = np.arange(1, 1000) / 1000.0
    assert (ic._pow_numba(t, 3) != ic._pow_libm(t, 3)).any() and np.array_equal(ic._pow_numba(t, 2), ic._pow_libm(t, 2))
    assert np.max(np.abs(ic._pow_numba(t, 3) - ic._pow_libm(t, 3)) / np.spacing(ic._pow_libm(t, 3))) <= 1.0


@pytest.mark.parametrize("rows", list(ic.ROWS))
def test_the_kernels_formulation_is_the_emulation_bit_for_bit(rows):
    book = ic.pairs(rows)
    assert len(set(book)) == len(book)
    for n, m in book:
        w = ic.rows_of(rows, n).astype(ic.LOOPS[rows])
        for mode in ic.modes_for(rows, n, m):
            assert _same(ic.model(w, mode, m), ic.want(rows, n, m, mode)), (rows, n, m, mode)


def test_what_the_book_holds():
    f32 = ic.pairs("f32")
    ns = {n for n, _ in f32}
    assert set(ic.SMALL + ic.SWITCH["f32"] + ic.LOADER) <= ns and max(n for n in ns if n < 5000) < 3100
    for mode, esz, rows in (("l", 4, "f32"), ("s", 4, "f32"), ("l", 8, "f64"), ("s", 8, "f64")):
        sw = [n for n in ic.SWITCH[rows] if ic.wide(mode, n, esz) != ic.wide(mode, n - 1, esz) or ic.wide(mode, n, esz) != ic.wide(mode, n + 1, esz)]
        assert len(sw) == 2, (mode, rows, sw)  # both sides of the narrow / wide switch
        top = ic.limit(mode, rows)
        assert {top, top - 1} <= {n for n, _ in ic.pairs(rows)}
    ratios = {(m / n) for n, m in f32}
    assert {1.0, 2.0, 10.0, 16.0, 0.5} <= ratios and any(m == 1 for _, m in f32) and any(m == n - 1 for n, m in f32) and any(m == n + 1 for n, m in f32)
    assert any(3 * n + 1 >= 2 * m >= 3 * n for n, m in f32) and any(m == 7 * n // 3 for n, m in f32) and any(m == max(4 * n // 9, 1) for n, m in f32)
    for pair in ic.NAMED_PAIRS:
        assert pair in f32
    # the float64 bound expression is not the rational one: at i = 7 for (14, 58), i = 15 for (18, 150), and the nearest rule's for (7, 58)
    # (bound(i) = ceil(u (i + 1)): index 6 is i = 7 of the reference's i_in + 1; the last bound, past the row, differs too and fills nothing)
    assert np.flatnonzero(ic.bounds("f", 14, 58) != ic.rational_bounds("f", 14, 58))[0] == 6
    assert np.flatnonzero(ic.bounds("f", 18, 150) != ic.rational_bounds("f", 18, 150))[0] == 14
    assert (ic.bounds("n", 7, 58) != ic.rational_bounds("n", 7, 58)).any()
    for mode, (n, m) in ic.FLOAT_BOUND_PAIRS.items():
        d = np.flatnonzero(ic.bounds(mode, n, m) != ic.rational_bounds(mode, n, m))
        assert len(d) and 0 < d[0] < n - 1 and (n, m) in f32
    fams = ic.FLOAT_FAMILIES
    assert {f"nan-{p}" for p in ("first", "middle", "last")} <= set(fams)
    assert {f"{s}inf-{p}" for s in "+-" for p in ("first", "middle", "last")} <= set(fams)


def _caught(rows, variant, modes, warm=ic.WARM):
    """the (n, m, mode) of the book where the wrong neighbour differs from the emulation"""
    out = []
    for n, m in ic.pairs(rows):
        if n > 3100:
            continue
        w = ic.rows_of(rows, n).astype(ic.LOOPS[rows])
        for mode in ic.modes_for(rows, n, m):
            if mode in modes and not _same(ic.model(w, mode, m, variant=variant, warm=warm), ic.want(rows, n, m, mode)):
                out.append((n, m, mode))
    return out


def test_the_wrong_neighbours_the_book_catches():
    got = _caught("f32", "rational", "nfclhs")
    # a bound computed rationally: in every mode whose value jumps at a bound ('l' is continuous there: t = 1 of one segment is t = 0 of the next)
    assert {mode for _, _, mode in got} >= set("nfchs")
    assert (14, 58, "f") in got and (18, 150, "f") in got and (7, 58, "n") in got
    assert len(_caught("f32", "s-upper-segment", "s")) > 20  # a segment one off at a bound in 's': wherever a bound is an output
    assert len(_caught("f32", "h-tail-clamped", "h")) > 20  # 'h''s tail not extrapolated
    assert _caught("f32", "l-diff-f64", "l")  # 'l''s float32 difference taken in float64 (the noise rows: not integers)
    assert not _caught("i16", "l-diff-f64", "l")  # (integer rows: the difference is exact either way -- what lets the reference's body pin the loop)
    short = _caught("f32", None, "s", warm=8)  # a warm-up of 8
    assert short and all(n > 8 for n, _, _ in short)
