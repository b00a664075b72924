"""The case book of the waveform aligner (tests/align_cases.py) against the reference bodies' recorded results (tests/golden/align.npz,
tools/gen_golden_align.py, the bodies run with numba's typing): the emulation -- the yardstick of the GPU tests -- equals the reference bit for
bit on every case the reference defines.  These are integer copies and single roundings: no tolerance.  A row on which the reference raised in
NumPy is one the book marks as undefined, and the other way round; their share stays below one in five, and every defined branch keeps its
cases."""
import json
import os

import numpy as np
import pytest

import align_cases as ac

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"{ac.BOOK}.npz")
ALIGN_LENGTHS, CORRECTION_LENGTHS = (2, 3, 40, 129), (3, 65, 129)


@pytest.fixture(scope="module")
def book():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def index(book):
    return {e["case"]: e for e in json.loads(str(book["__index__"]))}


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def test_the_fixture_holds_data_only_and_every_case(book, index):
    for loop in ac.LOOPS:
        assert {f"centroid_{loop}_n{n}" for n in ac.LENGTHS} <= set(index)
        assert {f"align_{loop}_n{n}_size{p[2]}" for n in ALIGN_LENGTHS for p in ac.align_params(n)} <= set(index)
        assert {f"correct_{loop}_n{n}_p{k}" for n in CORRECTION_LENGTHS for k in range(len(ac.correction_params(n)))} <= set(index)
        assert {f"inl_{loop}_{c[0]}" for c in ac.inl_cases(loop)} <= set(index)
    assert os.path.getsize(GOLDEN) < 600 * 1024
    assert all(v.dtype.kind in "fi" or k == "__index__" for k, v in book.items())


@pytest.mark.parametrize("loop", ["f32", "f64"])
def test_get_wf_centroid(book, loop):
    T, undefined, total, sums = ac.LOOPS[loop], 0, 0, {0: 0, 1: 0}
    for n in ac.LENGTHS:
        names, rows = ac.centroid_rows(loop, n)
        ref, status = book[f"centroid_{loop}_n{n}/out"], book[f"centroid_{loop}_n{n}/status"]
        for k, shift in enumerate(ac.centroid_shifts(n)):
            mine, defined = ac.emulate_centroid(rows, shift, T)
            assert np.array_equal(status[k] == ac.NUMPY_ERROR, ~defined) and not (status[k] == ac.FATAL).any(), (n, shift)
            assert np.isnan(mine[~defined]).all()  # the device's rule
            assert same(mine[defined], ref[k][defined]), (n, shift, [names[i] for i in np.flatnonzero(defined) if not mine[i] == ref[k][i]])
            undefined, total = undefined + int((~defined).sum()), total + len(defined)
            if float(shift) == int(shift):  # the parities of c_a + c_b, where a tie can come up
                for r in np.flatnonzero(defined & ~np.isnan(mine)):
                    w = rows[r]
                    lo, hi = int(np.argmin(w)), int(np.argmax(w))
                    parity = (lo + np.flatnonzero(w[lo:hi] > 0)[0] + lo + np.flatnonzero(w[lo:hi] < 0)[-1]) % 2
                    sums[int(parity)] += 1
    assert undefined * 5 < total and undefined > 0, (undefined, total)
    assert min(sums.values()) >= 3, sums
    # the issue's measurement: minimum at 12, maximum at 26 -> 19, 22, 22 for shifts 0, 3, 2.5; and a tie that goes down, one that goes up
    names, rows = ac.centroid_rows(loop, 65)
    r = names.index("measured")
    assert (int(np.argmin(rows[r])), int(np.argmax(rows[r]))) == (12, 26)
    ref = book[f"centroid_{loop}_n65/out"]
    assert [ref[k][r] for k in range(3)] == [19, 22, 22] and ac.centroid_shifts(65)[:3] == (0.0, 3.0, 2.5)
    assert ref[0][names.index("odd-18.5")] == 18 and ref[0][names.index("odd-19.5")] == 20


@pytest.mark.parametrize("loop", ["f32", "f64"])
def test_wf_alignment(book, index, loop):
    T, undefined, total, branches = ac.LOOPS[loop], 0, 0, {"window": 0, "pad": 0, "head": 0}
    for n in ALIGN_LENGTHS:
        names, rows = ac.align_rows(loop, n)
        rows = np.concatenate([rows, rows[:1]])
        for s in sorted({p[2] for p in ac.align_params(n)}):
            ref, status = book[f"align_{loop}_n{n}_size{s}/out"], book[f"align_{loop}_n{n}_size{s}/status"]
            params = [p for p in ac.align_params(n) if p[2] == s]
            assert len(params) == len(ref)
            for k, (c, sh, _s) in enumerate(params):
                cs = np.full(len(rows), c, T)
                cs[-1] = np.nan
                mine, st = ac.emulate_alignment(rows, cs, sh, s, T)
                assert np.array_equal(st, status[k]), (n, c, sh, s)
                assert np.isnan(mine[st != ac.OK]).all()  # the device's rule where the reference raises in NumPy; the fatal row's output is nobody's
                assert same(mine[st == ac.OK], ref[k][st == ac.OK]), (n, c, sh, s)
                assert st[-1] == ac.FATAL and (st[:-1] != ac.FATAL).all()
                undefined, total = undefined + int((st == ac.NUMPY_ERROR).sum()), total + len(st)
                win = ac.align_window(T(c), T(sh), s, n)
                if win is not None:
                    branches[win[0]] += 1
            assert index[f"align_{loop}_n{n}_size{s}"]["note"] == "centroid is nan"
    assert undefined * 5 < total and undefined > 0, (undefined, total)
    assert min(branches.values()) >= 3, branches
    # the issue's measurements: c = 3.7, s = 10 and c = -6, sh = 15 fail in NumPy's broadcast; integral centroids with k > 0 agree
    assert ac.align_window(3.7, 8.0, 10, 40) is None and ac.align_window(-6.0, 15.0, 10, 40) is None
    assert ac.align_window(3.0, 8.0, 10, 40) == ("pad", 2, 8) and ac.align_window(3.0, 8.0, 9, 40) == ("pad", 2, 7) and ac.align_window(-2.0, 8.0, 10, 40) == ("pad", 7, 3)
    # the two typings: CPython refuses a float slice bound, numba truncates it
    with pytest.raises(TypeError):
        ac.emulate_alignment(rows, 5.0, 0.0, 10.0, T, typing="cpython")
    assert same(ac.emulate_alignment(rows, 5.0, 0.0, 10.0, T)[0], ac.emulate_alignment(rows, 5.0, 0.0, 10, T, typing="cpython")[0])


@pytest.mark.parametrize("loop", ["f32", "f64"])
def test_integer_rows_align_like_their_values(loop):
    T = ac.LOOPS[loop]
    for dtype in (np.uint16, np.int16, np.int32):
        _, rows = ac.align_rows(loop, 40, dtype)
        for c, sh, s in ac.align_params(40)[::7]:
            a, sa = ac.emulate_alignment(rows, c, sh, s, T)
            b, sb = ac.emulate_alignment(rows.astype(T), c, sh, s, T)
            assert same(a, b) and np.array_equal(sa, sb)


@pytest.mark.parametrize("loop", ["f32", "f64"])
def test_wf_correction(book, index, loop):
    T = ac.LOOPS[loop]
    for n in CORRECTION_LENGTHS:
        _, rows = ac.correction_rows(loop, n)
        for k, (m, start, stop, nan_at) in enumerate(ac.correction_params(n)):
            ref, status = book[f"correct_{loop}_n{n}_p{k}/out"], book[f"correct_{loop}_n{n}_p{k}/status"]
            assert (status == ac.OK).all()
            mine = ac.emulate_correction(rows, ac.template(loop, m, nan_at), start, stop, T)
            assert same(mine, ref), (n, m, start, stop, nan_at)
            if nan_at is not None:
                assert np.isnan(ref).all()
    for k, (n, m, start, stop, text) in enumerate(ac.CORRECTION_REFUSALS):
        e = index[f"correct_refused_{loop}_{k}"]
        assert e["fatal"] and e["note"] == text.replace("\\", "")


@pytest.mark.parametrize("loop", ["f32", "f64"])
def test_inl_correction(book, index, loop):
    T = ac.LOOPS[loop]
    for name, rows, p, nan_at in ac.inl_cases(loop):
        ref, status = book[f"inl_{loop}_{name}/out"], book[f"inl_{loop}_{name}/status"]
        mine, st, text = ac.emulate_inl(rows, ac.inl_table(loop, p, nan_at), T)
        assert np.array_equal(st, status), name
        assert same(mine[st == ac.OK], ref[st == ac.OK]), name
        assert index[f"inl_{loop}_{name}"]["note"] == (text or ""), name
    e = index[f"inl_{loop}_code-p"]
    assert e["note"] == "ADC code 256 out of range for INL array of length 256" and index[f"inl_{loop}_code-negative"]["note"] == "ADC code -4 out of range for INL array of length 256"
    assert np.isnan(book[f"inl_{loop}_nan-table-code-p/out"]).all() and not book[f"inl_{loop}_nan-table-code-p/status"].any()
    if loop == "f32":  # one rounding of the float64 sum, not two float32 ones
        rows, table = ac.inl_cases(loop)[7][1], ac.inl_table(loop, ac.INL_BIG)
        once = book["inl_f32_big-i32/out"]
        twice = rows.astype(np.float32) + table[rows]
        assert ac.inl_cases(loop)[7][0] == "big-i32" and (once != twice).any()


def test_step(book):
    for loop, T in ac.LOOPS.items():
        for n in (1, 2, 3, 4, 10, 16, 17):
            assert same(ac.emulate_step(n, T), book[f"step_{loop}_n{n}/out"])
    assert list(np.flatnonzero(ac.emulate_step(10) == 1)) == [3, 4, 5, 6, 7] and list(np.flatnonzero(ac.emulate_step(16) == 1)) == list(range(4, 12))
