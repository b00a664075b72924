"""Records tests/golden/energy_row_pipeline.npz: the register-resident energy kernel's outputs, on the device, for the seeded inputs of
tests/test_gpu_energy_row_pipeline.py (the guard cases and the row-loop launches of tests/energy_row_pipeline_cases.py).

    python tools/record_energy_row_pipeline_fixture.py [OUT.npz]        (DSPEED_HIP_LIB selects the library that is recorded)

The test compares the kernel with this file EXACTLY.  It was recorded with the library as it stood before the guard reads of the lagged
streams were given addresses of their own, and it is recorded again only when the kernel's arithmetic is changed on purpose -- never to
make a failing comparison pass.  The row-loop launches depend on the device's launch geometry (rows per round = its wavefronts): the
file carries those numbers, and the test says so when it meets another."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_energy_row_pipeline as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    rec = {}
    for case in T.GUARD_CASES:
        for mode in case[5]:
            rec[f"guard/{case[0]}/{mode}"] = T.run_guard_case(case, mode)
    strides = {w: T.loop_stride(w) for w in T.R.LOOP_GEOMETRY}
    for w, stride in strides.items():
        rec[f"loop/stride-{w}"] = np.int64(stride)
    for lid in T.LOOP_IDS:
        rec[f"loop/{lid}"] = T.run_loop_launch(lid, strides)[3]
    np.savez_compressed(out, **rec)
    print(f"{len(rec)} outputs -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
