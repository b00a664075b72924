"""Writes tests/golden/histogram.npz: the rows of tests/histogram_cases.py with what the REFERENCE's own bodies of histogram
(processors/histogram.py:14-89) and histogram_stats (processors/histogram_stats.py:157-261) return for them, and -- for the general rows of
the float32 loop, which numba and NumPy 2 type differently (histogram_cases.py says how) -- the explicit emulation of numba's typing as the
expectation, with the body's NumPy-2 result beside it as numpy2_*.

    python tools/gen_golden_histogram.py

Runs only where the reference checkout is (oracle/gen_golden.py knows where: its numba stub and importer are used as they are).  Fails if a
row holds an infinity, or makes either rule set index k >= len(weights_out): the reference defines nothing there.  On the exact rows and in
the float64 loop the emulation must reproduce the body bit for bit, or the generator fails.
Per group and number of bins m: m<m>_x (the exact rows), m<m>_weights, m<m>_borders, m<m>_stats (mode, max, fwhm of histogram_stats with max_in
NaN on those outputs), m<m>_numpy2_weights / _borders (the general rows only: on the exact ones the body is the expectation)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import histogram_cases as hc  # noqa: E402
from oracle import gen_golden  # noqa: E402


def same(a, b):
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def run_stats(body, wt, ed, max_in, T):
    out = [np.zeros(1, dtype=T) for _ in range(3)]
    with np.errstate(invalid="ignore"):
        body(wt, ed, out[0], out[1], out[2], T(max_in))
    return [o[0] for o in out]


def main():
    gen_golden._install_stubs()
    hist = gen_golden._ref("histogram").histogram
    stats = gen_golden._ref("histogram_stats").histogram_stats
    book = gen_golden.Book(hc.BOOK)
    for g in hc.groups():
        T = g.loop
        arrays = {"w": g.w}
        for m in g.ms:
            rows, exact = g.rows(m), g.exact(m)
            assert not np.isinf(rows.astype(np.float64)).any(), (g.name, "an infinite sample")
            R = len(rows)
            weights, borders = np.zeros((R, m), dtype=T), np.zeros((R, m + 1), dtype=T)
            body_w, body_b = np.zeros((R, m), dtype=T), np.zeros((R, m + 1), dtype=T)
            st = np.zeros((R, 3), dtype=T)
            for r in range(R):
                x = rows[r].astype(T)
                with np.errstate(invalid="ignore", over="ignore"):
                    hist(x, body_w[r], body_b[r])  # (k >= m: IndexError, and no fixture)
                weights[r], borders[r], kmax = hc.numba_rules(x, m, T)
                assert kmax < m, (g.name, m, r, "k >= m under numba's rules")
                if exact[r] or T is np.float64:
                    assert same(weights[r], body_w[r]) and same(borders[r], body_b[r]), (g.name, m, r, "the emulation misses the body")
                    weights[r], borders[r] = body_w[r], body_b[r]
                st[r] = run_stats(stats, weights[r], borders[r], np.nan, T)
            arrays.update({hc.key(m, "x"): g.x[m], hc.key(m, "weights"): weights, hc.key(m, "borders"): borders, hc.key(m, "stats"): st})
            if T is np.float32:
                arrays.update({hc.key(m, "numpy2_weights"): body_w[~exact], hc.key(m, "numpy2_borders"): body_b[~exact]})  # (the general rows)
        book.add(g.name, hc.KERNEL, g.tag, arrays, params={"n": g.n, "rows": g.names, "ms": g.ms, "rows_dtype": np.dtype(g.rows_dtype).name})
    for name, tag, m, W, E, M, names in hc.stats_groups():
        T = W.dtype.type
        out = np.array([run_stats(stats, W[r], E[r], M[r], T) for r in range(len(W))], dtype=T)
        book.add(name, hc.KERNEL_STATS, tag, {"weights": W, "edges": E, "max_in": M, "stats": out}, params={"m": m, "rows": names})
    book.save()


if __name__ == "__main__":
    main()
