"""Do the cases of multi_time_point_thresh and time_over_threshold say something?  On the fixtures alone (tests/golden/thresholds.npz: the
rows of threshold_cases.py with what the reference's bodies returned), no GPU: the book is what the generator builds and holds every family
the kernel can go wrong on; the NumPy model of the kernel's formulation -- the thresholds ranked, the two merged walks 64 samples a step,
wrap-around reads -- returns the expectation on every case, bit for bit; and the model of m independent walks does not."""
import os

import numpy as np
import pytest

import golden_util
import threshold_cases as tc


@pytest.fixture(scope="module")
def book():
    return golden_util.cases(tc.BOOK, kernel=tc.KERNEL)


@pytest.fixture(scope="module")
def built():
    return {g.name: g for g in tc.groups()}


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def test_the_book_is_what_the_generator_builds(book, built):
    assert sorted(built) == sorted(c.name for c in book)
    for c in book:
        g = built[c.name]
        assert _same(c["w"], g.w) and _same(c["thr"], g.thr) and _same(c["ts"], g.ts) and _same(c["tot_thr"], g.tot_thr)
        assert c.params["rows"] == g.names and c.params["n"] == g.n and c.params["m"] == g.m and c.dtype == g.loop
        assert [tuple(x) for x in c.params["combos"]] == g.combos and c.params["shared"] == g.shared
        for pol, mode in g.combos:
            assert c[tc.key(pol, mode)].shape == (len(g.w), g.m) and c[tc.key(pol, mode)].dtype == g.loop
        assert c["tot"].shape == (len(g.w),) and c["tot"].dtype == g.loop
    # under the size of the other processors' fixtures
    assert os.path.getsize(os.path.join(golden_util.GOLDEN_DIR, tc.BOOK + ".npz")) <= 560 * 1024


def test_the_book_holds_every_family(book):
    for tag in ("f32", "f64"):
        mine = [c for c in book if c.tag == tag]
        assert {c.params["n"] for c in mine} == set(tc.LENGTHS)
        assert {c.params["m"] for c in mine} == set(tc.MS)
        assert {(p, m) for c in mine for p, m in map(tuple, c.params["combos"])} == {(p, m) for p in tc.POLARITIES for m in tc.MODES}
        names = [nm.split(":") for c in mine for nm in c.params["rows"]]
        assert {f for f, _, _ in names} == set(tc.FAMILIES)
        assert {k for _, k, _ in names} == set(tc.LISTS) | {"shared"}
        assert {s for _, _, s in names} == set(tc.STARTS) | {"shared"}
        assert any(c.params["shared"] for c in mine) and any(not c.params["shared"] for c in mine)
    assert {c.params["rows_type"] for c in book} == {"f32", "f64", "i16", "u16"}
    for c in book:
        w, thr, ts, n = c["w"], c["thr"], c["ts"], c.params["n"]
        for r, nm in enumerate(c.params["rows"]):
            family, kind, start = nm.split(":")
            if family == "nan_last" and c.params["rows_type"] in ("f32", "f64"):
                assert np.isnan(w[r, -1]) and not np.isnan(w[r, :-1]).any()
            if family == "constant":
                assert np.ptp(w[r]) == 0
            if family == "ties":
                assert np.all(w[r] == np.rint(w[r])) and np.ptp(w[r].astype(np.float64)) <= 10
            if kind == "nan":
                assert np.isnan(thr[r]).sum() == 1
            if kind == "inf":
                assert np.isinf(thr[r]).any()
            if kind == "dup" and c.params["m"] >= 3:
                assert len(np.unique(thr[r])) < c.params["m"]
            a = w[r, int(ts[r])] if 0 <= ts[r] < n else np.nan
            if kind == "above" and not np.isnan(a):
                assert np.all(thr[r] >= a)
            if kind == "below" and not np.isnan(a):
                assert np.all(thr[r] < a)
            if start in ("neg", "n", "nan"):
                assert not 0 <= ts[r] < n
            if start == "half":
                assert ts[r] != np.floor(ts[r])


def test_every_group_of_rows_finds_times(book):
    """in every (polarity sign, mode, loop) group at least a third of the rows hold a finite time"""
    found, rows = {}, {}
    for c in book:
        for pol, mode in map(tuple, c.params["combos"]):
            k = (pol > 0, mode, c.tag)
            t = c[tc.key(pol, mode)]
            found[k] = found.get(k, 0) + int(np.isfinite(t).any(axis=1).sum())
            rows[k] = rows.get(k, 0) + len(t)
    assert sorted(found) == sorted((s, m, t) for s in (False, True) for m in tc.MODES for t in ("f32", "f64"))
    for k in found:
        assert 3 * found[k] >= rows[k], (k, found[k], rows[k])


def test_the_model_of_the_kernel_is_the_reference(book):
    for c in book:
        T = c.dtype
        w = c["w"].astype(T)
        for pol, mode in map(tuple, c.params["combos"]):
            want = c[tc.key(pol, mode)]
            got = np.stack([tc.model(w[r], c["thr"][r], c["ts"][r], pol, mode, T) for r in range(len(w))])
            assert _same(got, want), (c.name, pol, mode, [c.params["rows"][r] for r in range(len(w)) if not _same(got[r], want[r])][:4])
        got = np.array([tc.model_time_over_threshold(w[r], c["tot_thr"][r], T) for r in range(len(w))], dtype=T)
        assert _same(got, c["tot"]), c.name


def test_the_walk_width_does_not_matter(book):
    """the merged walk is the reference's at any window: a sample a step, and 7 (no divisor of anything)"""
    for c in [c for c in book if c.params["n"] <= 129]:
        T = c.dtype
        w = c["w"].astype(T)
        pol, mode = c.params["combos"][1]
        for lanes in (1, 7):
            got = np.stack([tc.model(w[r], c["thr"][r], c["ts"][r], pol, mode, T, lanes=lanes) for r in range(len(w))])
            assert _same(got, c[tc.key(pol, mode)]), (c.name, lanes)


def test_independent_walks_are_not_the_reference(book):
    """The thresholds are a chain: on at least 20 rows m walks of their own give something else, all of them with polarity < 0."""
    differ = set()
    for c in book:
        T = c.dtype
        w = c["w"].astype(T)
        for pol, mode in map(tuple, c.params["combos"][:4]):  # (every polarity once: the mode changes the time, not where it is found)
            want = c[tc.key(pol, mode)]
            for r in range(len(w)):
                if not _same(tc.independent(w[r], c["thr"][r], c["ts"][r], pol, mode, T), want[r]):
                    assert pol < 0, (c.name, r, pol, mode)
                    differ.add((c.name, r))
    assert len(differ) >= 20, len(differ)


def test_wrapped_reads_are_in_the_book(book):
    """times below zero: the reference's reads of w[-1] and w[-2]"""
    negative = sum(int((c[tc.key(p, m)] < 0).sum()) for c in book for p, m in map(tuple, c.params["combos"]))
    assert negative >= 10, negative
