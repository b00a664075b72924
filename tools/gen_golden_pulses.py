"""Writes tests/golden/pulses.npz: what the REFERENCE's own bodies of peak_snr_threshold (processors/peak_snr_threshold.py) and
multi_a_filter (processors/multi_a_filter.py) return for tests/pulse_cases.py -- nothing of the product, nothing of the emulation.

    python tools/gen_golden_pulses.py

Runs only where the reference checkout is (oracle/gen_golden.py knows where: its numba stub and importer are used as they are).  The
bodies run under CPython.  multi_a_filter calls the gufunc fixed_time_pickoff on a list: the stub leaves that body a plain function of one
position, so it is applied here entry by entry in list order -- what the gufunc's broadcasting does --, and stops at the first DSPFatal.
Outputs only: rows, lists, ratios and widths come from the case book.  The lists multi_a_filter reads are the ones peak_snr_threshold
returned, as in the recipe ("va_max_out"), and the case's own list as it stands, NaNs in the middle included ("va_max_direct").  A row on
which multi_a_filter raises is marked in the case's "fatal" / "fatal_direct" array and its amplitudes are recorded as NaN; rows of the
classes the reference defines no result for (pulse_cases.EXEMPT) are not run through the picker: NaN lists, a count of 0."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import pulse_cases as pc  # noqa: E402
from oracle import gen_golden  # noqa: E402


def main():
    gen_golden._install_stubs()
    one_pickoff = gen_golden._ref("fixed_time_pickoff").fixed_time_pickoff

    def pickoff_over_a_list(w_in, t_in, mode_in, a_out):
        for j in range(len(t_in)):
            one_pickoff(w_in, t_in[j], mode_in, a_out[j:j + 1])

    sys.modules["dspeed.processors"].fixed_time_pickoff = pickoff_over_a_list
    picker = gen_golden._ref("peak_snr_threshold").peak_snr_threshold
    amplitudes = gen_golden._ref("multi_a_filter").multi_a_filter
    fatal_type = sys.modules["dspeed.errors"].DSPFatal
    book = gen_golden.Book(pc.BOOK)
    for loop, T in pc.LOOPS.items():
        for c in pc.all_cases(loop):
            R, m = len(c["rows"]), c["m"]
            idx, count = np.full((R, m), np.nan, T), np.zeros(R, np.uint32)
            amp, fatal = np.full((R, m), np.nan, T), np.zeros(R, np.uint8)
            direct, direct_fatal = np.full((R, m), np.nan, T), np.zeros(R, np.uint8)

            def pick_off(row, positions, out, mark, r):
                try:
                    amplitudes(row, positions, out[r])
                except fatal_type as e:
                    assert "fixed_time_pickoff requires integer t_in when using mode 'i'" in str(e)
                    mark[r], out[r] = 1, np.nan

            with np.errstate(all="ignore"):
                for r in range(R):
                    if m < c["n"]:  # the case's own list, NaNs where they stand: every position has a reference result
                        pick_off(c["rows"][r], c["lists"][r], direct, direct_fatal, r)
                    if c["exempt"][r]:
                        continue
                    picker(c["rows"][r], c["lists"][r], c["ratio"][r], T(c["width"]), idx[r], count[r:r + 1])
                    if m < c["n"]:
                        pick_off(c["rows"][r], idx[r], amp, fatal, r)
            arrays = {"idx_out": idx, "n_idx_out": count}
            if m < c["n"]:
                arrays.update(va_max_out=amp, fatal=fatal, va_max_direct=direct, fatal_direct=direct_fatal)
            book.add(c["key"], pc.KERNEL, loop, arrays, params={"n": c["n"], "m": m, "width": c["width"]})
    book.save()


if __name__ == "__main__":
    main()
