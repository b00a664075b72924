"""Writes tests/golden/thresholds.npz: the rows of tests/threshold_cases.py with what the REFERENCE's own bodies of multi_time_point_thresh
(processors/time_point_thresh.py:225-401) and time_over_threshold (processors/time_over_threshold.py:11-48) return for them -- nothing of
the product, nothing of the model.

    python tools/gen_golden_thresholds.py

Runs only where the reference checkout is (oracle/gen_golden.py knows where: its numba stub and importer are used as they are).  The
bodies are called as the gufuncs' loops would call them: integer rows cast to the loop's float type, thresholds as an array and t_start
and polarity as scalars of that type, the mode as an int8.  One case per group of rows; per (polarity, mode) the array t_<p|m><|polarity|>_<mode>,
and ``tot`` for time_over_threshold."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import threshold_cases as tc  # noqa: E402
from oracle import gen_golden  # noqa: E402


def main():
    gen_golden._install_stubs()
    multi = gen_golden._ref("time_point_thresh").multi_time_point_thresh
    over = gen_golden._ref("time_over_threshold").time_over_threshold
    book = gen_golden.Book(tc.BOOK)
    for g in tc.groups():
        T = g.loop
        arrays = {"w": g.w, "thr": g.thr, "ts": g.ts, "tot_thr": g.tot_thr}
        rows = g.w.astype(T)
        with np.errstate(all="ignore"):
            for pol, mode in g.combos:
                t_out = np.empty((len(rows), g.m), dtype=T)
                for r, w in enumerate(rows):
                    multi(w, g.thr[r], T(g.ts[r]), T(pol), np.int8(ord(mode)), t_out[r])
                arrays[tc.key(pol, mode)] = t_out
            tot = np.empty(len(rows), dtype=T)
            for r, w in enumerate(rows):
                over(w, T(g.tot_thr[r]), tot[r:r + 1])
            arrays["tot"] = tot
        book.add(g.name, tc.KERNEL, g.tag, arrays,
                 params={"n": g.n, "m": g.m, "rows_type": g.rows, "shared": bool(g.shared), "rows": g.names, "combos": [[p, m] for p, m in g.combos]})
    book.save()


if __name__ == "__main__":
    main()
