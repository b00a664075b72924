"""Writes tests/golden/spectrum.npz: what the REFERENCE's own bodies of fft and psd (processors/fft.py:12-46, 92-126) return for the rows
of tests/spectrum_cases.py -- nothing of the product, nothing of the model.

    python tools/gen_golden_spectrum.py

Runs only where the reference checkout is (oracle/gen_golden.py knows where: its numba stub and importer are used as they are).  The
bodies are called as the gufuncs' loops would call them: integer rows cast to the loop's float type, the output a complex64 / complex128
(fft) or float32 / float64 (psd) array of n // 2 + 1 bins.  Under the stub psd's helper ``abs2norm`` is the plain scalar function, not a
ufunc: it is wrapped here to run element by element on the scalars numba's signatures name (complex64, uint32 -> float32), its own body.
The rows themselves are not stored (they come from their seeds); of the long rows only the noise rows' spectra are, and psd only up
to 257 samples: the fixture stays small.  The float64 truth is nobody's fixture: every test computes it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import spectrum_cases as sc  # noqa: E402
from oracle import gen_golden  # noqa: E402


def main():
    gen_golden._install_stubs()
    ref = gen_golden._ref("fft")
    scalar_abs2norm = ref.abs2norm

    def abs2norm(x, norm, out):
        out[:] = [scalar_abs2norm(v, np.uint32(norm)) for v in x]

    ref.abs2norm = abs2norm
    book = gen_golden.Book(sc.BOOK)
    for g in sc.groups():
        T = g.loop
        C = np.complex64 if T is np.float32 else np.complex128
        m = g.n // 2 + 1
        arrays = {}
        if g.stored:
            rows = g.w[g.stored].astype(T)
            fft = np.empty((len(rows), m), dtype=C)
            psd = np.empty((len(rows), m), dtype=T)
            with np.errstate(all="ignore"):
                for r, w in enumerate(rows):
                    ref.fft(w, fft[r])
                    if g.with_psd:
                        ref.psd(w, psd[r])
            arrays["fft"] = fft
            if g.with_psd:
                arrays["psd"] = psd
        book.add(g.name, sc.KERNEL, g.tag, arrays, params={"n": g.n, "rows_type": g.rows, "rows": g.names, "stored": g.stored})
    book.save()


if __name__ == "__main__":
    main()
