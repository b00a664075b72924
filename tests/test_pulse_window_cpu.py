"""The window rule of dsp_pulses.hip on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program with a
``main`` of its own, plain g++, no HIP, nothing preloaded.

``tests/pulse_window.cpp`` includes ``dsp_kernels.h`` and holds the ``dsp_pulses`` namespace -- the bounds (a, b) of a candidate's window,
the dropped candidates, the clamped width: what the kernel and the planner share -- against the processor's loop for every row length up to
40, every candidate of the row with four fractions, and every width up to 45, and replays a lane's walk on an array as long as the row."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include")]


def test_the_window_and_a_lanes_walk_are_the_processors_loop(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    probe = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(probe) and os.path.exists(probe)):
        pytest.skip("g++ has no AddressSanitizer runtime here")
    exe = str(tmp_path / "pulse_window")
    subprocess.check_call(FLAGS + [os.path.join(ROOT, "tests", "pulse_window.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-6000:])
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    # every (n, c, fraction) whose candidate lies inside the row -- all of them: c + 0.999 < n for c <= n - 1 --, times 46 widths
    assert rep["failures"] == 0 and rep["triples"] == sum(n * 4 * 46 for n in range(1, 41)) and rep["dropped"] == 40 * 10
    assert rep["reads"] > rep["triples"]
    # the kernel and the planner use the same functions
    kernel = open(os.path.join(ROOT, "dspeed_amd", "csrc", "dsp_pulses.hip")).read()
    planner = open(os.path.join(ROOT, "dspeed_amd", "csrc", "dsp_plan.cpp")).read()
    assert "using namespace dsp_pulses;" in kernel and "dropped((double)vt, n)" in kernel and "window((double)vt, n, A.width)" in kernel
    assert "dsp_pulses::clamped_width(" in planner
