"""Writes tests/golden/spectrum_calls.json.gz: what every call of tests/test_spectrum_plan_cpu.py's case list hands to the library (against
the stand-in of tests/fake_dsp_lib.py), what it returns or raises.  No GPU, no reference.

    python tools/record_spectrum_calls.py
"""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_spectrum_plan_cpu as t  # noqa: E402


def main():
    book = {t.case_id(c): t.record(c) for c in t.CASES}
    with gzip.GzipFile(t.GOLDEN, "wb", mtime=0) as f:
        f.write(json.dumps(book, indent=1, sort_keys=True).encode())
    print(f"wrote {t.GOLDEN}: {len(book)} calls")


if __name__ == "__main__":
    main()
