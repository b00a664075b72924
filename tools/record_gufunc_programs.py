"""Records tests/golden/gufunc_programs.txt.gz: what tests/gufunc_programs.cpp prints -- the dsp_op program, io descriptors, io pointer order and
return code of every single-processor entry point (dspeed_amd/csrc/dsp_gufuncs.cpp), on the CPU, against stand-ins for the chain functions.

    python tools/record_gufunc_programs.py [OUT.txt.gz]           (zcat shows it)

tests/test_gufunc_programs_cpu.py compares the program's output with this file EXACTLY.  It was recorded from the entry points as they stood
in dsp_host.cpp, moved into dsp_gufuncs.cpp and otherwise untouched, before their builders were collapsed.  It is recorded again only when an
entry point is added or its program is changed on purpose -- never to make a failing comparison pass."""
import gzip
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gufunc_programs_cpu as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    with tempfile.TemporaryDirectory() as tmp:
        text = T.run_program(T.build_program(os.path.join(tmp, "gufunc_programs")))
    with open(out, "wb") as f, gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as z:  # (no name, no time: the same bytes every time)
        z.write(text.encode())
    print(f"{sum(1 for line in text.splitlines() if not line.startswith(' '))} records -> {out} ({len(text)} bytes)")


if __name__ == "__main__":
    main()
