"""Do the cases of histogram and histogram_stats say something?  On the fixtures alone (tests/golden/histogram.npz: the rows of
histogram_cases.py with what the reference's bodies returned, and the emulation of numba's typing for the general rows of the float32 loop),
no GPU: the book is what the generator builds and holds every family of rows the kernel can go wrong on, and the NumPy model of the kernel's
formulation returns the expectation on every case, bit for bit, for every number of samples per lane the kernels are built with."""
import os

import numpy as np
import pytest

import golden_util
import histogram_cases as hc


@pytest.fixture(scope="module")
def book():
    return golden_util.cases(hc.BOOK, kernel=hc.KERNEL)


@pytest.fixture(scope="module")
def stats_book():
    return golden_util.cases(hc.BOOK, kernel=hc.KERNEL_STATS)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _rows(c, m):
    x = c[hc.key(m, "x")]
    return np.concatenate([c["w"], x]) if len(x) else c["w"]


def test_the_book_is_what_the_generator_builds(book, stats_book):
    built = {g.name: g for g in hc.groups()}
    assert sorted(built) == sorted(c.name for c in book)
    for c in book:
        g = built[c.name]
        assert c["w"].dtype == g.w.dtype and np.array_equal(c["w"], g.w, equal_nan=True)
        assert c.params["rows"] == g.names and c.params["ms"] == g.ms and c.params["n"] == g.n and c.dtype == g.loop
        for m in g.ms:
            assert _same(c[hc.key(m, "x")], g.x[m])
            assert c[hc.key(m, "weights")].shape == (len(g.rows(m)), m) and c[hc.key(m, "borders")].shape == (len(g.rows(m)), m + 1)
    built = {name: rest for name, *rest in hc.stats_groups()}
    assert sorted(built) == sorted(c.name for c in stats_book)
    for c in stats_book:
        tag, m, W, E, M, names = built[c.name]
        assert _same(c["weights"], W) and _same(c["edges"], E) and _same(c["max_in"], M) and c.params["rows"] == names and c.params["m"] == m
    # well under the peak finder's fixture
    assert os.path.getsize(os.path.join(golden_util.GOLDEN_DIR, hc.BOOK + ".npz")) <= 560 * 1024


def test_the_book_holds_every_family(book, stats_book):
    f32 = [c for c in book if c.name.startswith("f32")]
    assert sorted(c.params["n"] for c in f32) == sorted(hc.LENGTHS)
    assert {m for c in f32 for m in c.params["ms"]} == set(hc.BINS) and all(100 in c.params["ms"] for c in book)
    assert {c.params["rows_dtype"] for c in book} == {"float32", "int16", "uint16", "float64"}
    for c in f32:
        names, w = c.params["rows"], c["w"]
        if c.params["n"] >= 3:
            for nm, at in (("nan_first", 0), ("nan_last", -1), ("nan_mid", c.params["n"] // 2)):
                if nm in names:
                    assert np.isnan(w[names.index(nm), at])
            assert "nan_mid" in names and "contention" in names and "max_many" in names
            r = w[names.index("contention")]
            assert (r == 7).sum() == len(r) - 2 and r.min() == 0 and r.max() == 100
            r = w[names.index("max_many")]
            assert (r == r.max()).sum() > 1 or c.params["n"] < 8
        if "constant" in names:
            assert np.ptp(w[names.index("constant")]) == 0 and set(np.unique(w[names.index("two_valued")])) <= {0, 1}
        assert not np.isinf(w).any()
        for m in c.params["ms"]:  # the exact rows: integers, range m * 2^j, both ends present; on the borders: every sample a border
            for x in c[hc.key(m, "x")]:
                assert np.array_equal(x, np.rint(x)) and np.abs(x).max() < 2 ** 24
                j = np.log2((x.max() - x.min()) / m)
                assert j == int(j)
    # the two rule sets differ somewhere among the general float32 rows (or the emulation would pin nothing the body does not)
    differs = sum(not _same(c[hc.key(m, "numpy2_borders")], c[hc.key(m, "borders")][: len(c["w"])]) for c in f32 for m in c.params["ms"])
    assert differs > 0
    # histogram_stats: max_in in all its cases, ties and zeros around the mode, NaN weights and edges
    for c in stats_book:
        kinds = {nm.rsplit("_", 1)[1] if not nm.endswith("past_end") else "past_end" for nm in c.params["rows"]}
        assert {"nan", "inside", "below", "beyond", "past_end"} <= kinds
        assert any(nm.startswith("plateau") for nm in c.params["rows"]) and any(nm.startswith("holes") for nm in c.params["rows"])
        assert any(nm.startswith("nan_edges") for nm in c.params["rows"]) and any(nm.startswith("nan_weight") for nm in c.params["rows"])
    assert {c.params["m"] for c in stats_book if c.tag == "f32"} == set(hc.BINS)
    found = np.concatenate([c["stats"][:, 2] for c in stats_book])
    assert np.isnan(found).any() and (found > 0).any()


@pytest.mark.parametrize("N", hc.LANE_SAMPLES)
def test_the_model_of_the_kernel_returns_the_expectation(book, N):
    n_rows = 0
    for c in book:
        if c.params["n"] == 8192 and N not in (1, 4):
            continue  # (the long rows with the widths float32 rows run on)
        for m in c.params["ms"]:
            rows, want_w, want_b = _rows(c, m), c[hc.key(m, "weights")], c[hc.key(m, "borders")]
            for r in range(len(rows)):
                got_w, got_b = hc.model_histogram(rows[r], m, c.dtype, N)
                assert _same(got_w, want_w[r]) and _same(got_b, want_b[r]), (c.name, m, r)
                n_rows += 1
    assert n_rows > 500


def test_the_weights_count_every_sample_but_the_maxima(book):
    for c in book:
        for m in c.params["ms"]:
            rows, wts, brd = _rows(c, m).astype(c.dtype), c[hc.key(m, "weights")], c[hc.key(m, "borders")]
            for r in range(len(rows)):
                if np.isnan(rows[r]).any():
                    assert not wts[r].any() and np.isnan(brd[r]).all()
                elif np.ptp(rows[r]) == 0:
                    assert not wts[r].any() and (brd[r] == rows[r][0]).all()
                else:
                    assert wts[r].sum() == (rows[r] != rows[r].max()).sum() and brd[r][0] == rows[r].min() and brd[r][-1] == rows[r].max()
                    assert (np.diff(brd[r].astype(np.float64)) >= 0).all()


def test_the_model_of_the_stats_returns_what_the_body_returned(book, stats_book):
    n_rows = 0
    for c in stats_book:
        W, E, M, want = c["weights"], c["edges"], c["max_in"], c["stats"]
        for r in range(len(W)):
            got = np.array(hc.model_stats(W[r], E[r], M[r], c.dtype), dtype=c.dtype)
            assert _same(got, want[r]), (c.name, c.params["rows"][r], got, want[r])
            n_rows += 1
    for c in book:  # and on the histograms themselves, as the fused launch computes them
        for m in c.params["ms"]:
            wts, brd, want = c[hc.key(m, "weights")], c[hc.key(m, "borders")], c[hc.key(m, "stats")]
            for r in range(len(wts)):
                got = np.array(hc.model_stats(wts[r], brd[r], np.nan, c.dtype), dtype=c.dtype)
                assert _same(got, want[r]), (c.name, m, r, got, want[r])
                n_rows += 1
    assert n_rows > 800


def test_an_infinity_is_a_nan_row():
    w = np.array([0.0, 1.0, np.inf, 2.0], dtype=np.float32)
    wts, brd = hc.model_histogram(w, 4, np.float32, 4)
    assert not wts.any() and np.isnan(brd).all()


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("n,m", [(16, 2), (1023, 4), (1024, 64), (8192, 64)])
def test_a_bin_index_that_reaches_m_is_dropped_and_nothing_else(T, n, m):
    """rows on which numba's rules give k = m for a known number of samples: neither rule set nor the model counts them anywhere, every other
    sample lands in its bin, and the model agrees for every number of samples per lane"""
    rows, want, dropped = hc.dropping_rows(n, m, T)
    for r in range(len(rows)):
        wts, _, kmax = hc.numba_rules(rows[r], m, T)
        assert (kmax >= m) == (dropped[r] > 0) and (kmax == m or dropped[r] == 0)
        assert np.array_equal(wts, want[r]) and wts.dtype == T
        assert (rows[r] != rows[r].max()).sum() - int(wts.sum()) == dropped[r]
        for N in hc.LANE_SAMPLES:
            got, brd = hc.model_histogram(rows[r], m, T, N)
            assert _same(got, want[r]) and brd[0] == rows[r].min() and brd[-1] == rows[r].max()
    # the row the guard is about in its smallest form: float32 [-1e8, 0.5, 1] with three bins
    w = np.array([-1e8, 0.5, 1.0], dtype=np.float32)
    wts, _, kmax = hc.numba_rules(w, 3, np.float32)
    assert kmax == 3 and list(wts) == [1, 0, 0] and list(hc.model_histogram(w, 3, np.float32, 1)[0]) == [1, 0, 0]
