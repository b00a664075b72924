"""Writes tests/golden/reflected_convolve.npz: what the REFERENCE's own bodies of reflected_convolve_wf (processors/convolutions.py) and
gaussian_filter1d (processors/gaussian_filter1d.py) return for the fixture's part of tests/reflect_cases.py -- nothing of the product,
nothing of the emulation.

    python tools/gen_golden_reflect.py

Runs only where the reference checkout is (oracle/gen_golden.py knows where: its numba stub and importer are used as they are).  Per case
the float32 body on the float32 rows ("f32"), the float64 body on the same float32 values ("f64_of_f32": the yardstick of the float32
loop's error) and, in the float64 loop, the float64 body ("f64").  Outputs only: rows and kernels come from the case book's seeds; the
Gaussian kernels of the cases are made by the reference's generator here and recorded, since the book's come from the product's."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import reflect_cases as rc  # noqa: E402
from oracle import gen_golden  # noqa: E402


def body_rows(fn, w, k, T):
    out = np.empty(w.shape, T)
    with np.errstate(all="ignore"):
        for r in range(len(w)):
            fn(w[r].astype(T), k.astype(T), out[r])
    return out


def main():
    gen_golden._install_stubs()
    conv = gen_golden._ref("convolutions").reflected_convolve_wf
    gauss = gen_golden._ref("gaussian_filter1d").gaussian_filter1d
    book = gen_golden.Book(rc.BOOK)
    for loop_name, T in (("f32", np.float32), ("f64", np.float64)):
        for key, n, m, name, k in rc.fixture_cases(loop_name):
            w = rc.rows_of(loop_name, n)
            if name == "gauss":  # the reference's own generator, with the scalars as its object-mode gufunc receives them
                lw = (m - 1) // 2
                k = np.empty(m, T)
                gauss(float(T(lw / 4 if lw else 0.1)), float(T(4)), k)
            arrays = {loop_name: body_rows(conv, w, k, T)}
            if T is np.float32:
                arrays["f64_of_f32"] = body_rows(conv, w, k, np.float64)
            if name == "gauss":
                arrays["kernel"] = k
            book.add(key, rc.KERNEL, loop_name, arrays, params={"n": n, "m": m, "kernel": name})
        for sigma, truncate in rc.GAUSS:
            lw = int(float(T(truncate)) * float(T(sigma)) + 0.5)
            k = np.empty(2 * lw + 1, T)
            gauss(float(T(sigma)), float(T(truncate)), k)
            book.add(f"gauss_{loop_name}_s{sigma}_t{truncate}", "host", loop_name, {"weights": k}, params={"sigma": sigma, "truncate": truncate})
    book.save()


if __name__ == "__main__":
    main()
