"""Writes tests/golden/get_multi_local_extrema.npz: the rows of tests/extrema_cases.py with what the REFERENCE's own body of
get_multi_local_extrema (processors/get_multi_local_extrema.py:12-306) returns for them -- nothing of the product, nothing of the model.

    python tools/gen_golden_extrema.py

Runs only where the reference checkout is (oracle/gen_golden.py knows where: its numba stub and importer are used as they are).  The
body is called as the gufunc's loops would call it: integer rows cast to the loop's float type, the four float parameters as scalars of
that type, uint32 counts.  One case per group of rows; per (search_direction, m) the arrays d<dir>_m<m>_{vt_max,vt_min,n_max,n_min}."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import extrema_cases as xc  # noqa: E402
from oracle import gen_golden  # noqa: E402


def main():
    gen_golden._install_stubs()
    body = gen_golden._ref("get_multi_local_extrema").get_multi_local_extrema
    book = gen_golden.Book(xc.BOOK)
    for g in xc.groups():
        T = g.loop
        arrays = {"w": g.w, "par": g.par.astype(T), **g.extra}
        rows = g.w.astype(T)
        for direction, m in g.combos:
            vt_max = np.empty((len(rows), m), dtype=T)
            vt_min = np.empty((len(rows), m), dtype=T)
            n_max = np.zeros(len(rows), dtype=np.uint32)
            n_min = np.zeros(len(rows), dtype=np.uint32)
            for r, w in enumerate(rows):
                p = [T(v) for v in g.par[:, r]]
                with np.errstate(invalid="ignore"):
                    body(w, p[0], p[1], direction, p[2], p[3], vt_max[r], vt_min[r], n_max[r:r + 1], n_min[r:r + 1])
            for what, a in (("vt_max", vt_max), ("vt_min", vt_min), ("n_max", n_max), ("n_min", n_min)):
                arrays[xc.key(direction, m, what)] = a
        book.add(g.name, xc.KERNEL, g.tag, arrays, params={"n": int(g.w.shape[1]), "rows": g.names, "combos": [list(c) for c in g.combos]})
    book.save()


if __name__ == "__main__":
    main()
