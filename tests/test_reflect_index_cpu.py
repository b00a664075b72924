"""The index and margin rules of dsp_reflect.hip on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program
with a ``main`` of its own, plain g++, no HIP, nothing preloaded.

``tests/reflect_index.cpp`` includes ``dsp_kernels.h`` and runs the ``dsp_reflect`` namespace -- the reflection, the margins, the layout of
the staged row in LDS and a lane's walk over it -- for every 1 <= m <= n <= 70 in both loops against the processor's formula, and the
limits' arithmetic at the edges of both geometries."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include")]


def test_the_staged_row_and_a_lanes_walk_are_the_formula(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    probe = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(probe) and os.path.exists(probe)):
        pytest.skip("g++ has no AddressSanitizer runtime here")
    exe = str(tmp_path / "reflect_index")
    subprocess.check_call(FLAGS + [os.path.join(ROOT, "tests", "reflect_index.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-6000:])
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    pairs = [(n, m) for n in range(1, 71) for m in range(1, n + 1)]
    assert rep["pairs"] == len(pairs) == 2485 and rep["failures"] == 0
    assert rep["outputs"] == sum(n for n, _m in pairs)
    assert rep["products"] == 2 * sum(n * m for n, m in pairs)  # every product of every output, in both loops
