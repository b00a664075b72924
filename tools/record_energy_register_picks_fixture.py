"""Records tests/golden/energy_register_picks.npz: the register-resident energy kernel's outputs, on the device, for the seeded inputs of
tests/test_gpu_energy_register_picks.py (the cases of tests/energy_register_picks_cases.py).

    python tools/record_energy_register_picks_fixture.py [OUT.npz]        (DSPEED_HIP_LIB selects the library that is recorded)

The test compares the kernel with this file EXACTLY.  It was recorded with the library as it stood while the pick-off samples, the carries'
capture groups and their prefix sums were still fetched through LDS, and it is recorded again only when the kernel's arithmetic is changed
on purpose -- never to make a failing comparison pass."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_energy_register_picks as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    rec = {}
    for case in T.CASES:
        for mode in case[5]:
            rec[f"{case[0]}/{mode}"] = T.run_case(case, mode)
    np.savez_compressed(out, **rec)
    print(f"{len(rec)} outputs -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
