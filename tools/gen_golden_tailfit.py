"""Writes tests/golden/tailfit.npz: what the REFERENCE's own bodies of log_check (processors/log_check.py), of the gufunc poly_fit(length, deg)
returns, of poly_diff and of poly_exp_rms (processors/poly_fit.py) return for tests/tailfit_cases.py -- nothing of the product, nothing of the
emulation.

    python tools/gen_golden_tailfit.py

Runs only where the reference checkout is (oracle/gen_golden.py knows where: its numba stub and importer are used as they are).  The bodies
run under CPython, and under CPython with NumPy 2 ``float32 * int`` stays float32 where numba makes it float64 (float32 * int64).  So the
float32 loop's rows and coefficients are handed to the bodies of poly_fit, poly_diff and poly_exp_rms as float64 arrays holding the float32
values, and the outputs stay float32 arrays: every product and every sum is then float64, and ``mean += ...`` / ``rms += ...`` add a float64
into a float32 array in place -- the float64 loop, cast back.  That is the reference body run with numba's typing (the table in
tests/tailfit_cases.py).  log_check takes the loop's own type: NumPy and numba agree there.
The inverted matrix is recorded as this run's factory computed it ("fit_<loop>_n<n>_m<m>/inv"): np.linalg.inv is LAPACK's, and the last
bits of an ill-conditioned inverse are the library's.  Outputs only otherwise: rows and coefficients come from the case book.  poly_fit
leaves the output of a row with a NaN untouched: it starts as NaN here, which is the product's rule."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import tailfit_cases as tc  # noqa: E402
from oracle import gen_golden  # noqa: E402


def as_numba_sees(a, T):
    """the loop's values in float64 arrays"""
    return np.asarray(a).astype(T).astype(np.float64)


def main():
    gen_golden._install_stubs()
    log_check = gen_golden._ref("log_check").log_check
    ref = gen_golden._ref("poly_fit")
    book = gen_golden.Book(tc.BOOK)
    with np.errstate(all="ignore"):
        for loop, T in tc.LOOPS.items():
            for n in tc.LENGTHS:
                rows = tc.tail_rows(loop, n)
                out = np.empty(rows.shape, T)
                for r in range(len(rows)):
                    log_check(rows[r], out[r])
                book.add(f"log_{loop}_n{n}", tc.KERNEL, loop, {"out": out}, params={"n": n})
            for n, m in tc.fit_cases():
                fitter = ref.poly_fit(n, m - 1)
                (inv,) = [c.cell_contents for c in fitter.ufunc.__closure__ if isinstance(c.cell_contents, np.ndarray)]
                rows = tc.tail_rows(loop, n)
                logged = tc.emulate_log_check(rows, T)  # (the rows a fit is made of in the chain, beside the raw ones)
                for name, w in (("fit", rows), ("fitlog", logged)):
                    pars = np.full((len(w), m), np.nan, T)
                    for r in range(len(w)):
                        fitter.ufunc(as_numba_sees(w[r], T), pars[r])
                    book.add(f"{name}_{loop}_n{n}_m{m}", tc.KERNEL, loop, {"pars": pars, **({"inv": inv} if name == "fit" else {})}, params={"n": n, "m": m})
            for n in tc.LENGTHS:
                for m in tc.MS:
                    rows, pars = tc.residual_case(loop, n, m)
                    for name, body in (("diff", ref.poly_diff), ("exp", ref.poly_exp_rms)):
                        mean, rms = np.empty(len(rows), T), np.empty(len(rows), T)
                        for r in range(len(rows)):
                            body(as_numba_sees(rows[r], T), as_numba_sees(pars[r], T), mean[r:r + 1], rms[r:r + 1])
                        book.add(f"{name}_{loop}_n{n}_m{m}", tc.KERNEL, loop, {"mean": mean, "rms": rms}, params={"n": n, "m": m})
    book.save()


if __name__ == "__main__":
    main()
