"""Writes tests/golden/ml_layers.npz: what the REFERENCE's own bodies of the neural-network layers (processors/ml.py) return for the
fixture's part of tests/ml_cases.py -- nothing of the product, nothing of the emulation.

    python tools/gen_golden_ml.py

Runs only where the reference checkout is (oracle/gen_golden.py knows where: its numba stub and importer are used as they are).  The
fixture's rows and weights are integer-valued with every partial sum below 2^24, so that np.dot's summation order cannot matter: on them
the body's 'r' is what any correct float32 dot product gives, bit for bit.  CPython runs the activation gufuncs under NumPy 2's typing (a
Python float beside a float32 array stays float32) where numba promotes to float64: 'r' and 't' are the same under both and are stored
under their own names; the others are stored as ``numpy2_<activation>``, beside which tests/ml_cases.py's emulation has both typings.
Outputs only: rows and weights come from their seeds."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ml_cases as mc  # noqa: E402
from oracle import gen_golden  # noqa: E402


def main():
    gen_golden._install_stubs()
    ml = gen_golden._ref("ml")
    book = gen_golden.Book(mc.BOOK)
    for n, m in mc.FIXTURE_SHAPES:
        x64, w64, b64 = mc.fixture_layer(n, m)
        for loop, T in (("f32", np.float32), ("f64", np.float64)):
            x, w, b = x64.astype(T), w64.astype(T), b64.astype(T)
            arrays = {}
            for act in mc.ACTIVATIONS + mc.UNKNOWN:
                name = act if act in "rt" + mc.UNKNOWN or T is np.float64 else f"numpy2_{act}"
                dense, dense_b = np.empty((len(x), m), T), np.empty((len(x), m), T)
                one, one_b = np.empty((len(x), 1), T), np.empty((len(x), 1), T)
                with np.errstate(all="ignore"):
                    for r in range(len(x)):
                        ml.dense_layer_no_bias(x[r], w, ord(act), dense[r])
                        ml.dense_layer_with_bias(x[r], w, b, ord(act), dense_b[r])
                        ml.classification_layer_no_bias(x[r], w[:, 0], ord(act), one[r])
                        ml.classification_layer_with_bias(x[r], w[:, 0], b[0], ord(act), one_b[r])
                arrays.update({f"dense/{name}": dense, f"dense_bias/{name}": dense_b, f"class/{name}": one[:, 0], f"class_bias/{name}": one_b[:, 0]})
            normed = np.empty_like(x)
            mu, var = (a.astype(T) for a in mc.fixture_norm(n))
            for r in range(len(x)):
                ml.normalisation_layer(x[r], mu, var, normed[r])
            arrays["normalised"] = normed
            book.add(f"{loop}_n{n}_m{m}", mc.KERNEL, loop, arrays, params={"n": n, "m": m})
    book.save()


if __name__ == "__main__":
    main()
