"""Writes tests/golden/interp_upsampler.npz: what the REFERENCE's own body of interpolating_upsampler (processors/upsampler.py:52-216)
returns for the fixture's part of tests/interp_cases.py -- nothing of the product, nothing of the emulation.

    python tools/gen_golden_interp.py

Runs only where the reference checkout is (oracle/gen_golden.py knows where: its numba stub and importer are used as they are).  The body
runs as written for all seven modes; what it cannot do under plain NumPy is mended on the data side, in the array handed to it as w_out:
an ndarray subclass that truncates the float slice bound of mode 'i' (``w_out[i_out+1 : i_out+upsample]``, numba's unsafe conversion) and
ignores the store at index len(w_out) that mode 's' begins with (an unchecked store one past the end under numba).
  * the float64 loop: rows of any kind, float64 in and out;
  * the float32 loop: integer-valued rows (every ADC row), given as a float64 copy and stored through a float32 w_out -- on such rows the
    float32 differences of numba's typing are exact, so the loop is the body on the copy with one rounding at the store.
CPython computes x**3 and x**2 with C's pow where numba unrolls products: tests/interp_cases.py's emulation has both, and this fixture
pins the pow one.  The rows themselves are not stored (they come from their seeds)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import interp_cases as ic  # noqa: E402
from oracle import gen_golden  # noqa: E402


class Out(np.ndarray):
    """w_out: float slice bounds truncated, a store at len(self) ignored"""

    def __setitem__(self, key, value):
        if isinstance(key, slice):
            key = slice(*(int(b) if isinstance(b, float) else b for b in (key.start, key.stop, key.step)))
        elif isinstance(key, (int, np.integer)) and key == len(self):
            return
        super().__setitem__(key, value)


def main():
    gen_golden._install_stubs()
    body = gen_golden._ref("upsampler").interpolating_upsampler
    book = gen_golden.Book(ic.BOOK)
    for n, m in ic.fixture_pairs():
        for loop, T in (("f64", np.float64), ("f32", np.float32)):
            rows = ic.fixture_rows(loop, n).astype(np.float64)
            arrays = {}
            for mode in ic.modes_of(n, m):
                out = np.empty((len(rows), m), dtype=T)
                with np.errstate(all="ignore"):
                    for r, w in enumerate(rows):
                        body(w, ord(mode), out[r].view(Out))
                arrays[mode] = out
            book.add(f"{loop}_n{n}_m{m}", ic.KERNEL, loop, arrays, params={"n": n, "m": m, "modes": ic.modes_of(n, m)})
    book.save()


if __name__ == "__main__":
    main()
